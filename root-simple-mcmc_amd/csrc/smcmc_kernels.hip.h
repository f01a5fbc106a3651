// smcmc_kernels.hip.h -- gfx950 kernels of the many-chain Metropolis step.
//
// One chain per lane, one 64-chain group per wavefront, one wavefront per
// workgroup (the headline's instantiations: four, SHARED in step_kernel).  A launch advances every chain by `nsteps` calls of
// sMCMC::TSimpleMCMC::Step() (reference TSimpleMCMC.H:370-496) without touching
// HBM between the steps: the accepted point lives in LDS as x[dim][lane]
// (conflict-free column per lane), the proposal in registers.
//   A  scalar half of TProposeAdaptiveStep::UpdateState (TSimpleMCMC.H:1723-1776)
//      per lane; in POOLED mode the current point is folded into the group's
//      second-moment accumulator with v_mfma_f64_16x16x4_f64 whose operands are
//      read straight from the LDS image of x (y = x - c0 formed on the fly),
//      replacing the per-chain running covariance of TSimpleMCMC.H:1780-1820
//   B  proposal x' = x + sigma U^T r (TSimpleMCMC.H:709-724), r from Philox +
//      Box-Muller (include/smcmc_detmath.h), U through wave-uniform scalar loads;
//      StepRMS window (:391-406); likelihood (:410); Metropolis test (:432-463);
//      accept copy (:484-491) as an exec-masked LDS write
// EXACT = the reference's un-fused operation order (mul, then add); !EXACT =
// fused multiply-add.  Both are reproduced bit for bit by oracle/ensemble_oracle.c.
//
// Runtime dim <= DP: state rows >= dim are zero, U / Error are zero padded, so the
// padded lanes of the arithmetic only ever add +-0 and need no guards.
//
// Compile with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "smcmc.h"
#include "smcmc_detmath.h"
#include "smcmc_event_sample.h"
#include "smcmc_step_deal.h"

namespace smcmc {

// Register-array sizes the step kernel is instantiated for, smallest first (an
// engine of dimension D runs the smallest DP >= D).  D + 1 <= 64 keeps the
// moment contraction within 4 x 4 tiles.  build.py reads this list.
#define SMCMC_FOR_EACH_DP(X) X(7) X(15) X(31) X(47) X(50) X(63)

#define SMCMC_DP_ENTRY(n) n,
constexpr int kDpMacroList[] = {SMCMC_FOR_EACH_DP(SMCMC_DP_ENTRY)};
#undef SMCMC_DP_ENTRY
constexpr bool dp_lists_agree() {
    if (sizeof(kDpMacroList) / sizeof(kDpMacroList[0]) != (size_t)kNumDpFamilies) return false;
    for (int f = 0; f < kNumDpFamilies; ++f)
        if (kDpMacroList[f] != kDpFamilies[f]) return false;
    return true;
}
static_assert(dp_lists_agree(), "kDpFamilies of smcmc_step_deal.h restates SMCMC_FOR_EACH_DP: keep the two alike");

constexpr int kWave = 64;
// (kXStride, the doubles per LDS row of the accepted point, lives with its layout: XLayout of smcmc_step_deal.h)

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Wave-uniform read-only tables (U, Error, c0) are read through the constant
// address space so that the loads become scalar (s_load into SGPRs, one fetch per
// wavefront through the scalar cache) instead of 64 identical vector loads.
typedef const __attribute__((address_space(4))) double* cptr_f64;
typedef const __attribute__((address_space(3))) double* lds_cptr_f64;
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) f64x2* lds_cptr_f64x2;
__device__ __forceinline__ cptr_f64 as_const(const double* p) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    return (cptr_f64)p;
#pragma clang diagnostic pop
}


// smcmc_normal_pair (smcmc_detmath.h) with its two tables in LDS: the index differs from lane to lane, which LDS serves
// in a few passes and a global load in up to 64 cache-line requests.  lt / at: 64 entries of two doubles each.
// The two entries come in ahead of the arithmetic (normal_tables_fetch): an LDS read returns in issue order, so a
// table read issued behind the prefetch of the next U piece would wait for the whole piece.
struct NormalTables { f64x2 le, ae; };
// Hand-placed LDS reads (inline assembly, waited for by hand: load_piece below says why) are only used where the
// compiler leaves them alone.  It sees an assembly read's destination as an ordinarily defined value and may copy or
// spill it at once -- before the data has arrived.  The families up to 31 dimensions, which it allocates for two
// wavefronts per SIMD, are short of registers and did exactly that (v_accvgpr_write right behind the read); they keep
// reads the compiler can see and count.  build.py runs inflight_check.py over every step-kernel listing and fails on
// a compiler instruction that touches a register with an assembly read in flight.
template <int DP>
constexpr bool kAsmReads = DP >= 47;
// LSH, ASH: log2 of the bytes from an entry to the next (4: one copy of a table; the headline kernels' replicated tables,
// NormalTableLayout, have the lane's copy in lt_base / at_base and a wider stride: the same shift-and-add)
template <bool ASM, int LSH = 4, int ASH = 4>
__device__ __forceinline__ NormalTables normal_tables_fetch(uint32_t w0, uint32_t w1, uint32_t lt_base, uint32_t at_base) {
    NormalTables t;
    const uint32_t la = lt_base + (smcmc_normal_log_index(w0) << LSH), aa = at_base + (smcmc_normal_angle_index_halfcircle(w1) << ASH);
    if constexpr (ASM) {
        asm volatile("ds_read_b128 %0, %1" : "=v"(t.le) : "v"(la));
        asm volatile("ds_read_b128 %0, %1" : "=v"(t.ae) : "v"(aa));
    } else {
        t.le = *(volatile lds_cptr_f64x2)(uintptr_t)la;
        t.ae = *(volatile lds_cptr_f64x2)(uintptr_t)aa;
    }
    return t;
}
template <int N, bool ASM>
__device__ __forceinline__ void normal_tables_ready(NormalTables& a, NormalTables& b) {
    if constexpr (ASM) asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a.le), "+v"(a.ae), "+v"(b.le), "+v"(b.ae) : "n"(N));
}
template <int N, bool ASM>
__device__ __forceinline__ void normal_tables_ready(NormalTables& a) {
    if constexpr (ASM) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a.le), "+v"(a.ae) : "n"(N));
}
__device__ __forceinline__ void normal_pair_lds(uint32_t w0, uint32_t w1, const NormalTables& t, double* n0, double* n1) {
#ifdef SMCMC_NORMAL_TEXTBOOK
    (void)t;   // the frozen-definition build (include/smcmc_detmath.h): the textbook pair, no tables
    smcmc_normal_pair(w0, w1, n0, n1);
    return;
#endif
#define SMCMC_LT_LDS(k, c) (t.le[c])
#define SMCMC_AT_LDS(c) (t.ae[c])
    SMCMC_NORMAL_PAIR_BODY_HALFCIRCLE(SMCMC_LT_LDS, SMCMC_AT_LDS)
#undef SMCMC_LT_LDS
#undef SMCMC_AT_LDS
}

// compile-time loop: f(std::integral_constant<int, 0>) ... f(<N-1>)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for_impl(F& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for_impl<I + 1, N>(f);
    }
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl<0, N>(f); }

// kPiece columns of row i starting at column c (c - j0(i) is even: 16-byte aligned reads).
//
// The reads are inline assembly and so is the wait for them.  A lone wavefront pays an issue slot (four cycles) for
// every instruction of any kind; left to the compiler, every use of a loaded pair gets a wait with a count of its own
// -- eight per piece, some 600 s_waitcnt per step, 7 % of the step.  LDS reads return in issue order, so ONE
// `s_waitcnt lgkmcnt(n)` placed after the next piece's n reads covers the whole current piece (piece_ready).  The
// compiler does not count reads it cannot see: its own waits then over-wait (safe), these wait for everything older
// (safe whatever else is in flight).
template <int DP, bool FULLU, int i, int c, int k = 0>
__device__ __forceinline__ void load_piece(uint32_t ubase, f64x2 (&dst)[kPiece / 2]) {
    typedef ULayout<DP, FULLU> UL;
    if constexpr (k < kPiece / 2) {
        if constexpr (c + 2 * k < UL::DPE) {
            constexpr int off = (UL::off(i) + (c - UL::j0(i)) + 2 * k) * 8;
            if constexpr (kAsmReads<DP>) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[k]) : "v"(ubase), "n"(off));
            else dst[k] = *(lds_cptr_f64x2)(uintptr_t)(ubase + (uint32_t)off);
        }
        load_piece<DP, FULLU, i, c, k + 1>(ubase, dst);
    }
}
// every LDS read older than the N youngest has returned; `piece` is the piece those older reads filled (its first M pairs)
template <int N, int M, bool ASM>
__device__ __forceinline__ void piece_ready(f64x2 (&q)[kPiece / 2]) {
    static_assert(kPiece == 16 && N >= 0 && N < 16 && M >= 1 && M <= 8, "eight register pairs per piece, a 4-bit counter");
    if constexpr (!ASM) return;
    else if constexpr (M == 8) asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]) : "n"(N));
    else if constexpr (M == 7) asm volatile("s_waitcnt lgkmcnt(%7)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]) : "n"(N));
    else if constexpr (M == 6) asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]) : "n"(N));
    else if constexpr (M == 5) asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]) : "n"(N));
    else if constexpr (M == 4) asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]) : "n"(N));
    else if constexpr (M == 3) asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]) : "n"(N));
    else if constexpr (M == 2) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(q[0]), "+v"(q[1]) : "n"(N));
    else asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(q[0]) : "n"(N));
}

// The matrix-pipe operands of one k-quad (four chains) of the moment fold, fetched one k-quad ahead: T raw values of the
// accepted point per lane (plus the strip's), inline assembly like the piece reads -- issued in the middle of a piece,
// covered by the next piece's piece_ready, consumed pieces later (operands_ready ties them behind that wait).  Read and
// used on the spot they cost the LDS latency sixteen times per step.
// KQ: bytes from a k-quad's four lanes of the image to the next one's (4 * 8 * XLayout::LANE).
template <int T, int KK, int KQ, int t = 0>
__device__ __forceinline__ void fetch_operands(const uint32_t (&xaddr)[T], double (&raw)[T]) {
    if constexpr (t < T) {
        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(raw[t]) : "v"(xaddr[t]), "n"(KQ * KK));
        fetch_operands<T, KK, KQ, t + 1>(xaddr, raw);
    }
}
template <int KK, int KQ>
__device__ __forceinline__ void fetch_operand(uint32_t addr, double& raw) {
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(raw) : "v"(addr), "n"(KQ * KK));
}
template <int T, int t = 0>
__device__ __forceinline__ void operands_ready(double (&raw)[T], double& raws) {
    if constexpr (t < T) {
        asm volatile("" : "+v"(raw[t]));
        operands_ready<T, t + 1>(raw, raws);
    } else {
        asm volatile("" : "+v"(raws));
    }
}

struct StepParams {
    int nchains, npad, dim;
    int nsteps, metropolis;
    uint32_t step0;            // fTotalSteps before this launch
    uint32_t chain_offset;
    uint64_t seed;
    const double* U;           // [DP][DP], zero padded
    const double* like;        // QUADFORM: Error [DP][DP] zero padded; ROSENBROCK: {b}
    const int32_t* like_rowptr;   // QUADFORM with a sparse Error: its non-zero entries (QuadCsr below), else nullptr
    const int32_t* like_cols;
    const double* like_vals;
    const int32_t* like_rows;
    const double* c0;          // [DP] centre the moments are taken about
    double target, acc_window, asig, max_up;
    double acc_w, acc_wW;      // acceptance de-weighting: w = 1 - deweight, w*window; acc_w < 0 = off
    int per_lane_update;       // FROZEN mode: per-chain UpdateProposal schedule
    int step_rms_window;
    int has_forced;            // ForceStep pending: the first step proposes `forced`
    const double* forced;      // [DP][npad]
    double* x;                 // [DP][npad], rows >= dim stay zero
    double* lane_f64;          // [SMCMC_LANE_F64_COUNT_][npad]
    int32_t* lane_i32;         // [SMCMC_LANE_I32_COUNT_][npad]
    double* gacc;              // [group][NT][4][64] moment accumulators
    double* save_x;            // optional [slot][DP][npad]
    double* save_logl;         // optional [slot][npad]
    int save_stride;
    uint64_t uniform_mask;     // bit d: dimension d has a uniform proposal (TSimpleMCMC.H:711-716)
    const double* uniform;     // [2][DP]: lower bounds, upper bounds
    int scan_dim;              // fScanDimension (TSimpleMCMC.H:685-704), -1 = off
    int scan_uniform;          // the scanned dimension has a uniform proposal
    double scan_a, scan_b;     // uniform: bounds; Gaussian: centre, sigma
    double* proposed;          // optional [DP][npad]: the proposal of the launch's last step (fProposed, TSimpleMCMC.H:576);
                               // the SPECIAL instantiation and the fused-order kernels look at it
    int zero;                  // always 0; makes table addresses depend on the step so that the
                               // compiler does not hoist (and then spill) whole tables out of the loop
    unsigned long long* prof;  // section profile (SMCMC_STEP_PROFILE builds only): [group][kProfSlots][64] cycle sums, added to
    int like_lds_bytes;        // SMCMC_LIKE_EVENT_SAMPLE / _TEMPLATE / _SHAPE: dynamic LDS of the launch, the lanes' histograms (event_sample_lds_bytes, event_shape_lds_bytes)
    double* like_park;         // SMCMC_LIKE_EVENT_TEMPLATE / _SHAPE: the park image [3 or 4 nbins][npad] (event_two_pass_loglike)
};

// ---- Section profile of the step loop: -DSMCMC_STEP_PROFILE=1 (sections) or 2 (sections and every piece) ----
// Never in the shipped library (tools/micro/build_stepprof.sh builds a second one with one object replaced).  The step
// loop takes s_memtime stamps at section boundaries; the cycles since the previous stamp go to the section that ends
// there.  The sums live in lanes of vector registers -- lane k of slot 0 is section k, lane g & 63 of slots 1 .. 6 is
// piece g (its read drain, its arithmetic, its matrix part; two slots each: pieces 0-63, 64-127; the full-matrix kernels'
// later pieces fold onto these) -- and leave through
// ordinary stores at the end of the launch.  A stamp waits for its own value (lgkmcnt(0)), which also drains the LDS
// queue: behind a stamp nothing is in flight, so a section never pays for the one before it, and what a piece's reads
// cost from issue to arrival shows in the piece's "drain" figure instead of hiding under the arithmetic.  The stamp's
// own cost is section PROF_STAMP (two stamps back to back, once per step); tools/micro/stepprof.py subtracts it.
constexpr int kProfSlots = 7;
enum { PROF_LOOP, PROF_STAMP, PROF_A, PROF_TOP, PROF_NORMALS, PROF_PIECES, PROF_TAIL, PROF_RMS, PROF_LIKE, PROF_TEST,
       PROF_COMMIT, PROF_ENDWAIT, PROF_COUNT };
enum { PROF_PIECE_DRAIN, PROF_PIECE_VALU, PROF_PIECE_MATRIX };
#ifdef SMCMC_STEP_PROFILE
struct StepProf {
    uint64_t last, slot[kProfSlots];
    __device__ __forceinline__ static uint64_t stamp() {
        uint64_t t;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t));
        __builtin_amdgcn_sched_barrier(0);
        return t;
    }
    __device__ __forceinline__ void start() {
#pragma unroll
        for (int q = 0; q < kProfSlots; ++q) slot[q] = 0;
        last = stamp();
    }
    template <int S>
    __device__ __forceinline__ void add(int k, int lane) {
        const uint64_t t = stamp();
        slot[S] += (lane == k) ? t - last : 0;
        last = t;
    }
};
#define SMCMC_PROF_MARK(k) prof.add<0>(k, lane)
#if SMCMC_STEP_PROFILE >= 2
#define SMCMC_PROF_PIECE(kind, g) prof.add<1 + 2 * (kind) + (((g) >> 6) & 1)>((g) & 63, lane)
#else
#define SMCMC_PROF_PIECE(kind, g)
#endif
#else
#define SMCMC_PROF_MARK(k)
#define SMCMC_PROF_PIECE(kind, g)
#endif

__device__ __forceinline__ double dmin(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ double dmax(double a, double b) { return __builtin_fmax(a, b); }

// A user likelihood compiled into the library (SMCMC_LIKE_USER): the header named by
// SMCMC_USER_LIKELIHOOD defines
//     template <int DP> __device__ double smcmc_user_loglike(const double (&p)[DP], smcmc::cptr_f64 params, int D);
// p[0..D) is the point (entries past D are zero), params what smcmc_set_likelihood_params handed over.
// For 63 < dim <= 512 the point does not fit one lane's registers; a header that also defines
//     #define SMCMC_USER_LIKELIHOOD_ANY_DIM 1
//     template <class Point> __device__ double smcmc_user_loglike_at(const Point& p, const double* params, int D);
// (p[i], 0 <= i < D, reads coordinate i of the chain's point from its [dim][chain] image in device memory) is served at
// those dimensions too, in reference-order arithmetic.
// A header with the any-dimension form may also give the HMC engine a gradient of its own (the OptionalGradient of
// TSimpleHMC<UserLikelihood, OptionalGradient>, TSimpleHMC.H:79-89):
//     #define SMCMC_USER_GRADIENT 1
//     template <class Point> __device__ double smcmc_user_gradient_at(const Point& p, const double* params, int D, int i);
// returns component i of grad log L at p (what the reference functor writes to g[i]; the engine negates it, :486).  One
// component per call, because in hmc_step_kernel every wavefront owns a slice of the components of its 64 chains: all
// owners compute theirs at once, each lane reading its chain's point through the same view as smcmc_user_loglike_at.
// Bit parity with a host functor is a matter of keeping that functor's operation order inside one component.
#ifdef SMCMC_USER_LIKELIHOOD
}  // namespace smcmc
#include SMCMC_USER_LIKELIHOOD
namespace smcmc {
#if defined(SMCMC_USER_GRADIENT) && !defined(SMCMC_USER_LIKELIHOOD_ANY_DIM)
#error "SMCMC_USER_GRADIENT needs SMCMC_USER_LIKELIHOOD_ANY_DIM: HMC runs a user likelihood through smcmc_user_loglike_at"
#endif
#endif

// log-likelihood of the point p[0..D) held in registers.
template <int DP, int LIKE, bool EXACT>
__device__ __forceinline__ double loglike(const double (&p)[DP], cptr_f64 prm, int D) {
    double logl = 0.0;
    if constexpr (LIKE == SMCMC_LIKE_ISO_GAUSS) {
        // README.md:57-66: logL += - 0.5*p[i]*p[i]   (padded dims add -0)
#pragma unroll
        for (int i = 0; i < DP; ++i) {
            double t = -0.5 * p[i];
            if constexpr (EXACT) logl += t * p[i];
            else logl = SMCMC_FMA(t, p[i], logl);
        }
    } else if constexpr (LIKE == SMCMC_LIKE_QUADFORM) {
        // TDummyLogLikelihood.H:24-28: logL -= 0.5*p[i]*Error(j,i)*p[j].  prm holds the
        // TRANSPOSE of Error (prm[i][j] = Error(j,i)) so that the inner loop walks a
        // contiguous row; rows are fetched in 16-column pieces as for U.
#pragma unroll
        for (int i = 0; i < DP; ++i) {
            const double h = 0.5 * p[i];
#pragma unroll
            for (int jc = 0; jc < DP; jc += 16) {
                cptr_f64 ep = prm + i * DP + jc;
#pragma unroll
                for (int jj = 0; jj < 16; ++jj) {
                    const int j = jc + jj;
                    if (j < DP) {
                        const double e = ep[jj];
                        if constexpr (EXACT) logl -= h * e * p[j];
                        else logl = SMCMC_FMA(-(h * e), p[j], logl);
                    }
                }
            }
        }
    } else if constexpr (LIKE == SMCMC_LIKE_USER) {
#ifdef SMCMC_USER_LIKELIHOOD
        logl = smcmc_user_loglike<DP>(p, prm, D);
#endif
    } else if constexpr (LIKE == SMCMC_LIKE_ASYM) {
        // TAsymLogLikelihood.H:20-31 (the same arithmetic in both orders: there is nothing to fuse)
        const double positive = prm[0], negative = prm[1];
#pragma unroll
        for (int i = 0; i < DP; ++i) {
            if (i < D) {
                double a = p[i];
                a = (a < 0.0) ? a * negative : a * positive;
                logl += a;
            }
        }
    } else if constexpr (LIKE == SMCMC_LIKE_HORRIFIC) {
        // THorrificLogLikelihood.H:26-38: -1E+30 as soon as a coordinate leaves the unit box
        bool outside = false;
#pragma unroll
        for (int i = 0; i < DP; ++i) {
            if (i < D) {
                outside = outside || (__builtin_fabs(p[i]) > 1.0);
                logl += p[i];
            }
        }
        const double sigma = 0.01;
        const double natural = __builtin_sqrt(D * 4.0 / 12.0);
        logl /= natural;
        logl = -0.5 * logl * logl / sigma / sigma;
        logl = outside ? -1E+30 : logl;
    } else if constexpr (LIKE == SMCMC_LIKE_CONSTRAINED) {
        // example4/TConstrainedLikelihood.H:26-46; prm = {SummedValues, SummedConstraint, Expected[D], Prior[D]}
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < DP; ++i)
            if (i < D) sum += p[i];
        sum = (sum - prm[0]) / prm[1];
        logl -= 0.5 * sum * sum;
#pragma unroll
        for (int i = 0; i < DP; ++i) {
            if (i < D) {
                double v = p[i] - prm[2 + i];
                v /= prm[2 + D + i];
                logl -= 0.5 * v * v;
            }
        }
    } else {
        // THardLogLikelihood.H:60-64
        const double rb = prm[0];
#pragma unroll
        for (int i = 0; i < DP - 1; ++i) {
            if (i < D - 1) {
                if constexpr (EXACT) {
                    double a = (1.0 - p[i]);
                    double b = p[i + 1] - p[i] * p[i];
                    logl -= a * a + rb * b * b;
                } else {
                    double a = 1.0 - p[i];
                    double b = SMCMC_FMA(-p[i], p[i], p[i + 1]);
                    double t = SMCMC_FMA(rb * b, b, a * a);
                    logl -= t;
                }
            }
        }
    }
    return logl;
}

// ---- The likelihoods over a simulated event sample (smcmc.h; the arithmetic is include/smcmc_event_sample.h): one
// family, SMCMC_LIKE_EVENT_SAMPLE here, its two-pass members _TEMPLATE and _SHAPE below ----
// One chain per lane.  Every lane walks all events in order; the packed sample is wave-uniform and comes through the
// constant address space (a few scalar loads per event for the whole wavefront).  A lane's three histograms sit in
// dynamic LDS as hist[bin][lane], bins laid end to end (Close, Separated, DecayTag) and one more row behind them that
// takes the events a cut or the axis drops: a lane only ever touches its own banks, whatever bin it hits, and the
// update needs no predicate.  The family the likelihood is built for (dim = 9: pick_dp gives 15):
constexpr int kEsDP = 15;
constexpr int kEsLdsLimit = 160 * 1024;       // LDS of a gfx950 compute unit, all of which one workgroup may have
// static LDS of step_kernel<kEsDP, ...> at its largest (moment fold, full decomposition): point, decomposition, tables
constexpr int kEsStaticLds = 8 * (XLayout<kEsDP, true, false>::DOUBLES + ULayout<kEsDP, true>::SIZE + 384) + 64;
constexpr int event_sample_lds_bytes(int nbins) { return (3 * nbins + 1) * kWave * 8; }
static_assert(kEsStaticLds + event_sample_lds_bytes(SMCMC_EVENT_SAMPLE_MAX_BINS) <= kEsLdsLimit &&
              kEsStaticLds + event_sample_lds_bytes(SMCMC_EVENT_SAMPLE_MAX_BINS + 1) > kEsLdsLimit,
              "SMCMC_EVENT_SAMPLE_MAX_BINS (smcmc.h) is the largest nbins whose histograms fit one workgroup beside the kernel's static LDS");
// The read-modify-write of a bin is a dependent LDS chain (address, read, add, write).  kEsBatch events are corrected
// first -- (bin, weight) in registers --, then their bins are read together, added to in event order and written back
// in event order: the reads' latency is paid once per batch.  Two events of a batch that hit the same bin: the later
// one adds to the earlier one's sum (taken from its register, not from the read), so the order of additions into a bin
// is the event order.
constexpr int kEsBatch = 4;
template <int DP>
__device__ __forceinline__ double event_sample_loglike(const double (&p)[DP], cptr_f64 prm, double* hist, int lane) {
    static_assert(DP >= SMCMC_ES_DIM, "the nine systematic parameters");
    const int nev = (int)prm[SMCMC_ES_H_NEVENTS], nbins = (int)prm[SMCMC_ES_H_NBINS];
    const double xmin = prm[SMCMC_ES_H_XMIN], xmax = prm[SMCMC_ES_H_XMAX], range = prm[SMCMC_ES_H_RANGE];
    const double cut = prm[SMCMC_ES_H_CUT];
    double pt[SMCMC_ES_DIM];
#pragma unroll
    for (int i = 0; i < SMCMC_ES_DIM; ++i) pt[i] = p[i];
    smcmc_es_scalars s;
    smcmc_es_point_scalars(pt, prm[SMCMC_ES_H_EXPOSURE], prm[SMCMC_ES_H_TRUE_FAKES], prm[SMCMC_ES_H_TRUE_EFF],
                           prm[SMCMC_ES_H_TAN_FAKES], prm[SMCMC_ES_H_TAN_EFF], &s);
    const int rows = 3 * nbins;                 // row `rows`: the dropped events'
    double* const col = hist + lane;
    for (int r = 0; r <= rows; ++r) col[r * kWave] = 0.0;
    const cptr_f64 ev = prm + SMCMC_ES_HEADER + rows;
    for (int e0 = 0; e0 < nev; e0 += kEsBatch) {
        int idx[kEsBatch];
        double w[kEsBatch], v[kEsBatch];
#pragma unroll
        for (int u = 0; u < kEsBatch; ++u) {
            const bool in = e0 + u < nev;                                   // (wave-uniform)
            const cptr_f64 q = ev + (size_t)(in ? e0 + u : nev - 1) * SMCMC_ES_EVENT;
            const int cls = (int)q[4];
            const int b = smcmc_es_event_bin(q[0], q[1], q[2], q[3], cls >> 1, cls & 1, &s, nbins, xmin, xmax, range, cut);
            idx[u] = (in && b >= 0) ? b : rows;
            w[u] = (cls == 0) ? s.weight[0] : (cls == 1) ? s.weight[1] : (cls == 2) ? s.weight[2] : s.weight[3];
        }
#pragma unroll
        for (int u = 0; u < kEsBatch; ++u) v[u] = col[idx[u] * kWave];
#pragma unroll
        for (int u = 0; u < kEsBatch; ++u) {
#pragma unroll
            for (int j = 0; j < u; ++j) v[u] = (idx[j] == idx[u]) ? v[j] : v[u];
            v[u] = v[u] + w[u];
        }
#pragma unroll
        for (int u = 0; u < kEsBatch; ++u) col[idx[u] * kWave] = v[u];
    }
    // FakeLikelihood.H:53-78: the bins of Close, Separated, DecayTag, in that order
    const cptr_f64 data = prm + SMCMC_ES_HEADER;
    double logl = 0.0;
    for (int r = 0; r < rows; ++r) logl += smcmc_es_bin_term(data[r], col[r * kWave]);
    return logl;
}

// ---- SMCMC_LIKE_EVENT_TEMPLATE and SMCMC_LIKE_EVENT_SHAPE (smcmc.h): the two-pass members of the family ----
// Six histograms per lane do not fit (154 KB at 50 bins beside kEsStaticLds), so a lane has the NH histograms of ONE class
// -- hist[NH nbins + 1][lane], NH = 3 for the template and 4 for the shape -- and the fill runs twice: over the signal
// events [0, nsignal), then, the rows zeroed again, over the background events [nsignal, nevents), whose batches start at
// nsignal -- no batch straddles the classes.  Between the passes the lane sums its rows to the signal's integral and writes
// ws * S[r], the signal's share of every bin, to its column of the park image: park[r][chain] in device memory, a row one
// coalesced 512-byte store of the wavefront.  The bin sum reads the share back and adds wb * B[r].  A lane reads only what
// it wrote itself, in program order: no fence.  The image is scratch of one evaluation, no chain state.
//
// The shape's weight of an event is its class's weight times exp(shape), and the shape reads the lane's control value y[k]
// and slope[k] at an index k that the packed event carries: wave-uniform, but known only at run time, so a register array
// would go to scratch inside the event loop.  The tables sit in the dynamic LDS behind the histograms as table[row][lane]:
// rows [0, n) the control values, rows [n, 2 n - 1) the slopes of the class whose pass is running -- n = 13 and 25 rows
// for the signal, n = 11 and 21 rows for the background.  The family the shape is built for (dim = 31):
constexpr int kEshDP = 31;
constexpr int kEshTableRows = 2 * SMCMC_ESH_NS - 1;
static_assert(SMCMC_ESH_NS >= SMCMC_ESH_NB, "the signal's tables are the larger");
// static LDS of step_kernel<kEshDP, ...> at its largest (moment fold, full decomposition): point, decomposition, tables
constexpr int kEshStaticLds = 8 * (XLayout<kEshDP, true, false>::DOUBLES + ULayout<kEshDP, true>::SIZE + 384) + 64;
constexpr int event_shape_lds_bytes(int nbins) { return (4 * nbins + 1 + kEshTableRows) * kWave * 8; }
static_assert(kEshStaticLds + event_shape_lds_bytes(SMCMC_EVENT_SHAPE_MAX_BINS) <= kEsLdsLimit &&
              kEshStaticLds + event_shape_lds_bytes(SMCMC_EVENT_SHAPE_MAX_BINS + 1) > kEsLdsLimit,
              "SMCMC_EVENT_SHAPE_MAX_BINS (smcmc.h) is the largest nbins whose histograms and tables fit one workgroup beside the kernel's static LDS");
static_assert(SMCMC_EVENT_SHAPE_MAX_BINS >= 50, "example3's own 50 bins must fit: shrink the tables, not the histograms");
// the dynamic LDS of a launch and the largest nbins it is sized for, by likelihood
constexpr int event_lds_bytes(int like, int nbins) {
    return like == SMCMC_LIKE_EVENT_SHAPE ? event_shape_lds_bytes(nbins) : event_sample_lds_bytes(nbins);
}
constexpr int event_max_bins(int like) {
    return like == SMCMC_LIKE_EVENT_SHAPE ? SMCMC_EVENT_SHAPE_MAX_BINS : SMCMC_EVENT_SAMPLE_MAX_BINS;
}

// The fill of a lane's column `col` (zeroed by the caller) with the events [ebeg, nev) of `ev`, batches counted from ebeg:
// event_sample_loglike's loop, batch for batch, and for the two-pass likelihoods the one shared copy.  Not shared with
// the event sample, because the event sample calling a function here -- this one over [0, nevents), or one for the batch
// alone -- changed its step kernels' control flow (sixteen more scalar branches, other register numbers), and with its
// loop written out they are what they were, instruction for instruction (profiles/event_template_notes.md).
// SHAPE: eight doubles per event, four histograms and the weight multiplied by exp(shape); tab: this lane's column of the
// tables of the pass's class, nctl its number of control values (neither is read without SHAPE, nor is cut_very_close).
template <bool SHAPE>
__device__ __forceinline__ void event_fill(double* const col, const double* const tab, const int nctl, const cptr_f64 ev,
                                           const int ebeg, const int nev, const smcmc_es_scalars& s, const int nbins,
                                           const int rows, const double xmin, const double xmax, const double range,
                                           const double cut_very_close, const double cut) {
    constexpr int STRIDE = SHAPE ? SMCMC_ESH_EVENT : SMCMC_ES_EVENT;
    for (int e0 = ebeg; e0 < nev; e0 += kEsBatch) {
        int idx[kEsBatch];
        double w[kEsBatch], v[kEsBatch];
#pragma unroll
        for (int u = 0; u < kEsBatch; ++u) {
            const bool in = e0 + u < nev;                                   // (wave-uniform)
            const cptr_f64 q = ev + (size_t)(in ? e0 + u : nev - 1) * STRIDE;
            const int cls = (int)q[4];
            int b, k = 0, ks = 0;
            if constexpr (SHAPE) {
                k = (int)q[5];                                              // (wave-uniform; 0 <= k < nctl: es_pack)
                ks = (k < nctl - 1) ? k : nctl - 2;                         // (a clamped event at the last centre has no slope)
                b = smcmc_esh_event_bin(q[0], q[1], q[2], q[3], cls >> 1, cls & 1, &s, nbins, xmin, xmax, range, cut_very_close, cut);
            } else {
                b = smcmc_es_event_bin(q[0], q[1], q[2], q[3], cls >> 1, cls & 1, &s, nbins, xmin, xmax, range, cut);
            }
            idx[u] = (in && b >= 0) ? b : rows;
            w[u] = (cls == 0) ? s.weight[0] : (cls == 1) ? s.weight[1] : (cls == 2) ? s.weight[2] : s.weight[3];
            if constexpr (SHAPE) w[u] = smcmc_esh_weight(w[u], smcmc_esh_shape(tab[k * kWave], tab[(nctl + ks) * kWave], q[6], q[7] != 0.0));
        }
#pragma unroll
        for (int u = 0; u < kEsBatch; ++u) v[u] = col[idx[u] * kWave];
#pragma unroll
        for (int u = 0; u < kEsBatch; ++u) {
#pragma unroll
            for (int j = 0; j < u; ++j) v[u] = (idx[j] == idx[u]) ? v[j] : v[u];
            v[u] = v[u] + w[u];
        }
#pragma unroll
        for (int u = 0; u < kEsBatch; ++u) col[idx[u] * kWave] = v[u];
    }
}
// a class's integral from the lane's NH histograms
template <int NH>
__device__ __forceinline__ double event_integral(const double* col, int nbins) {
    double sum[NH];
    for (int k = 0; k < NH; ++k) {
        const double* h = col + (size_t)k * nbins * kWave;
        double v = 0.0;
        for (int b = 0; b < nbins; ++b) v += h[b * kWave];
        sum[k] = v;
    }
    return smcmc_et_integral(sum, NH);
}
// TFakeGP::GetPenalty of N control values in registers, the inverse kernel through the constant address space
template <int N>
__device__ __forceinline__ double event_shape_penalty(const double (&y)[N], const cptr_f64 kinv) {
    double penalty = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) penalty += smcmc_esh_gp_term(y[i], y[j], kinv[i * N + j]);
    }
    return penalty;
}
// this lane's column of the shape's tables: the control values y and the slopes between the centres c
template <int N>
__device__ __forceinline__ void event_shape_tables(double* const tab, const double (&y)[N], const cptr_f64 c) {
#pragma unroll
    for (int i = 0; i < N; ++i) tab[i * kWave] = y[i];
#pragma unroll
    for (int i = 0; i + 1 < N; ++i) tab[(N + i) * kWave] = smcmc_esh_slope(y[i], y[i + 1], c[i], c[i + 1]);
}
// The two-pass likelihood: zero, fill, integral, norm, park after pass 0, then the bin sum from park plus wb * col
// (example2/FakeLikelihood.H:64-89, example3/FakeLikelihood.H:68-102: the bins of [VeryClose,] Close, Separated, DecayTag,
// in that order) and the penalties.  The shape writes its tables before each pass and adds its two penalties after.
// park: this lane's column of the image, rows npad apart
template <int DP, bool SHAPE>
__device__ __forceinline__ double event_two_pass_loglike(const double (&p)[DP], cptr_f64 prm, double* hist, int lane,
                                                         double* park, size_t npad) {
    constexpr int DIM = SHAPE ? SMCMC_ESH_DIM : SMCMC_ES_DIM, NH = SHAPE ? 4 : 3;
    static_assert(DP >= DIM, "the nine systematic parameters, or the 31 parameters of example3");
    const int nev = (int)prm[SMCMC_ES_H_NEVENTS], nbins = (int)prm[SMCMC_ES_H_NBINS], nsig = (int)prm[SMCMC_ES_H_NSIGNAL];
    const double xmin = prm[SMCMC_ES_H_XMIN], xmax = prm[SMCMC_ES_H_XMAX], range = prm[SMCMC_ES_H_RANGE];
    const double cut = prm[SMCMC_ES_H_CUT], cut_very_close = SHAPE ? prm[SMCMC_ESH_H_CUT_VERY_CLOSE] : 0.0;
    double pt[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) pt[i] = p[i];
    smcmc_es_scalars s;
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
    const int rows = NH * nbins;                // row `rows`: the dropped events'
    double* const col = hist + lane;
    double* const tab = col + (size_t)(rows + 1) * kWave;       // (the shape's alone)
    const cptr_f64 ev = prm + (SHAPE ? SMCMC_ESH_EVENTS(nbins) : SMCMC_ES_HEADER + rows);
    double wb = 0.0;
#pragma nounroll
    for (int c = 0; c < 2; ++c) {               // (one copy of the fill's code)
        for (int r = 0; r <= rows; ++r) col[r * kWave] = 0.0;
        if constexpr (SHAPE) {
            if (c == 0) event_shape_tables<SMCMC_ESH_NS>(tab, ys, prm + SMCMC_ESH_CENTRE_S(nbins));
            else event_shape_tables<SMCMC_ESH_NB>(tab, yb, prm + SMCMC_ESH_CENTRE_B(nbins));
        }
        event_fill<SHAPE>(col, tab, c ? SMCMC_ESH_NB : SMCMC_ESH_NS, ev, c ? nsig : 0, c ? nev : nsig, s, nbins, rows, xmin, xmax,
                          range, cut_very_close, cut);
        const double norm = smcmc_et_norm(c ? pt[1] : pt[0], event_integral<NH>(col, nbins));
        if (c == 0)
            for (int r = 0; r < rows; ++r) park[(size_t)r * npad] = smcmc_et_mc_signal(norm, col[r * kWave]);
        else wb = norm;
    }
    const cptr_f64 data = prm + SMCMC_ES_HEADER;
    double logl = 0.0;
    for (int r = 0; r < rows; ++r)
        logl += smcmc_es_bin_term(data[r], smcmc_et_mc(park[(size_t)r * npad], wb, col[r * kWave]));
    if constexpr (SHAPE) {
        const double pen_b = event_shape_penalty<SMCMC_ESH_NB>(yb, prm + SMCMC_ESH_KINV_B(nbins));
        const double pen_s = event_shape_penalty<SMCMC_ESH_NS>(ys, prm + SMCMC_ESH_KINV_S(nbins));
        return smcmc_esh_penalties(logl, pt, pen_b, pen_s);
    } else {
        return smcmc_et_penalties(logl, pt[0], pt[1], pt[6], pt[7], pt[8]);
    }
}

// SPECIAL = the variant that also knows uniform per-dimension proposals, the scan of one dimension
// (TSimpleMCMC.H:685-716) and the read-back of the proposed point (:514); kept out of the common kernels, whose
// register allocation it disturbs.
// The quadratic form (TDummyLogLikelihood.H:24-28) of a point held in a column of LDS, xq[XL::row(j)] (XL: its
// XLayout): the D^2-term running sum needs every p[j] for every i, which a register array can only give to fully
// unrolled code (50 x 50 terms: minutes of compile time per kernel) -- a rolled outer loop indexes it
// dynamically and the compiler moves it to scratch memory.  From LDS the outer loop can stay rolled.
template <int DP, bool EXACT, typename XL>
__device__ __forceinline__ double loglike_quadform_lds(const double* xq, cptr_f64 prm) {
    double logl = 0.0;
#pragma nounroll
    for (int i = 0; i < DP; ++i) {
        const double h = 0.5 * xq[XL::row(i)];
        cptr_f64 ep = prm + i * DP;
#pragma unroll
        for (int j = 0; j < DP; ++j) {
            const double e = ep[j];
            const double pj = xq[XL::row(j)];
            if constexpr (EXACT) logl -= h * e * pj;
            else logl = SMCMC_FMA(-(h * e), pj, logl);
        }
    }
    return logl;
}

// The same sum over the entries of Error that are not zero (rows of Error^T in compressed form, made by the host when
// the matrix is sparse -- the reference's own TDummy matrix is the identity plus one correlated pair: 52 entries of 2 500
// at D = 50).  A skipped term is (h * 0) * p[j] = +-0 for finite h and p[j], and `logl -= +-0` leaves logl as it is (logl
// starts at +0 and x - y is never -0 unless x is): bit for bit the dense sum.  With a non-finite coordinate the skipped
// terms would be NaN -- but then the diagonal term of that coordinate (the host insists on a full diagonal) makes this
// sum non-finite too, and the caller falls back on the dense one.
struct QuadCsr {
    const int32_t* rowptr;     // nullptr: no compressed form, use the dense sum; else rowptr[0] = number of entries, padded to
                               // a multiple of kQuadChunk with zero entries (a zero entry is a skipped term: +-0)
    const int32_t* cols;       // [nnz] column j of entry k (Error^T(i, j) = Error(j, i)); entries row by row, j ascending
    const double* vals;        // [nnz]
    const int32_t* rows;       // [nnz] row i of entry k
};
constexpr int kQuadChunk = 8;  // entries fetched together: three scalar loads per chunk instead of three dependent ones per entry
typedef const __attribute__((address_space(4))) int32_t* cptr_i32;
__device__ __forceinline__ cptr_i32 as_const(const int32_t* p) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    return (cptr_i32)p;
#pragma clang diagnostic pop
}
template <bool EXACT, typename Point>
__device__ __forceinline__ double quadform_csr(const Point& point, const QuadCsr& q, int D) {
    const cptr_i32 rw = as_const(q.rows), cl = as_const(q.cols);
    const cptr_f64 vl = as_const(q.vals);
    const int nnz = as_const(q.rowptr)[0];
    double logl = 0.0;
    for (int k0 = 0; k0 < nnz; k0 += kQuadChunk) {
        int ri[kQuadChunk], ci[kQuadChunk];
        double e[kQuadChunk], pi[kQuadChunk], pj[kQuadChunk];
#pragma unroll
        for (int u = 0; u < kQuadChunk; ++u) {
            ri[u] = rw[k0 + u];
            ci[u] = cl[k0 + u];
            e[u] = vl[k0 + u];
        }
#pragma unroll
        for (int u = 0; u < kQuadChunk; ++u) {
            pi[u] = point(ri[u]);
            pj[u] = point(ci[u]);
        }
#pragma unroll
        for (int u = 0; u < kQuadChunk; ++u) {
            const double h = 0.5 * pi[u];
            if constexpr (EXACT) logl -= h * e[u] * pj[u];
            else logl = SMCMC_FMA(-(h * e[u]), pj[u], logl);
        }
    }
    (void)D;
    return logl;
}

// The headline's two instantiations (D = 50 family, iso-Gaussian, reference order, triangular decomposition, no uniform
// dimensions / scan; with and without the moment fold).  They run as ONE workgroup of kStepWaves wavefronts per CU
// (StepWorkgroupLds of smcmc_step_deal.h; step_launch_shape below is the host's side of it), every other instantiation
// as one wavefront per workgroup.
template <int DP, int LIKE, bool EXACT, bool FULLU, bool SPECIAL>
constexpr bool kStepHeadline = EXACT && !FULLU && !SPECIAL && DP == 50 && LIKE == SMCMC_LIKE_ISO_GAUSS;

template <int DP, int LIKE, bool EXACT, bool FULLU, bool MOMENTS, bool SPECIAL>
__global__ void __launch_bounds__((kStepHeadline<DP, LIKE, EXACT, FULLU, SPECIAL> ? kStepWaves * kWave : kWave),
                                  (kStepHeadline<DP, LIKE, EXACT, FULLU, SPECIAL> ? 1 : 2)) step_kernel(const StepParams p) {
    constexpr int T = Geo<DP>::T;
    constexpr int NT = Geo<DP>::NT;
    constexpr int NB = Geo<DP>::NB;
    typedef ULayout<DP, FULLU> UL;
    // The headline's two instantiations (D = 50 family, iso-Gaussian, reference order, triangular decomposition, no
    // uniform dimensions / scan; with and without the moment fold): what was measured on them alone is theirs alone, and
    // every other instantiation keeps its code instruction for instruction.
    constexpr bool HEADLINE = kStepHeadline<DP, LIKE, EXACT, FULLU, SPECIAL>;
    // PAIRS: the accepted point in row pairs (XLayout): reload, StepRMS batch and commit are 16-byte accesses on one base
    // address.  FIXED_AW: the accept word taken from the one Philox block that holds it for every dimension the family
    // serves (AcceptBlock).  A dimension outside that range does not reach this kernel: the engine launches family
    // pick_dp(dim) (smcmc_host.hpp), the smallest that holds dim, so dim lies above the family before.  Each part on
    // the symbol it gained on by itself (profiles/step_rowpairs_notes.md): the row pairs on both, the accept block with
    // the fold only -- alone it moved the kernel without the fold by less than the runs differ.
    constexpr bool PAIRS = HEADLINE;
    constexpr bool FIXED_AW = HEADLINE && MOMENTS && AcceptBlock<DP>::FIXED;
    typedef XLayout<DP, MOMENTS, PAIRS> XL;
    static_assert(!PAIRS || DP % 2 == 0, "a lane's 16-byte accesses cover whole row pairs of the point");
    // ZROW: the fold's tile rows past the ones row read the image's zero row (XLayout::ZERO_ROW) instead of being clamped
    // onto the ones row and zeroed by a select, two selects per k-quad and double (profiles/step_rms_blocks_notes.md).
    // With the fold only: the other image has no such row.
    constexpr bool ZROW = HEADLINE && MOMENTS;
    static_assert(!ZROW || XL::ZERO_ROW == DP + 1, "the ones row's partner is the zero row");
    // SHARED: one workgroup of kStepWaves wavefronts per CU.  Wavefront w of block b is chain group kStepWaves b + w and
    // has an image of the accepted point of its own, which no other wavefront touches: its LDS operations on it execute
    // in issue order, so what BOUNDARY (below) says of the lone wavefront holds for it.  The decomposition and the
    // tables of the normal transform are held ONCE, staged by all the threads in front of the one barrier of the kernel;
    // the LDS that frees holds the tables in copies, so that a gather cannot conflict (NormalTableLayout;
    // profiles/step_shared_tables_notes.md).  A wavefront past the last group stages, reaches the barrier and ends.
    constexpr bool SHARED = HEADLINE;
    typedef StepWorkgroupLds<DP, MOMENTS> WL;
    static_assert(!SHARED || (PAIRS && WL::FITS && WL::IMAGE_BYTES == XL::BYTES), "the wavefronts' images lie end to end, within the CU's LDS");
    __shared__ alignas(PAIRS ? 16 : 8) double xs_own[SHARED ? 2 : XL::DOUBLES];   // accepted point, x[row][lane]
    __shared__ __attribute__((aligned(16))) double us_own[SHARED ? 2 : UL::SIZE];   // decomposition, every lane reads the same word
    __shared__ __attribute__((aligned(16))) double ntab_own[SHARED ? 2 : 384];      // tables of the normal transform: log [64][2], angle over the half circle [128][2]
    constexpr int NTHREADS = SHARED ? kStepWaves * kWave : kWave;
    int wave = 0;
    if constexpr (SHARED) wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double* xs = xs_own;
    double* us = us_own;
    double* ntab = ntab_own;
    if constexpr (SHARED) {
        extern __shared__ __attribute__((aligned(16))) double wg_lds[];
        xs = wg_lds + (WL::IMAGE_BYTES / 8) * wave;
        us = wg_lds + WL::US / 8;
        ntab = wg_lds + WL::LOG / 8;
    }

    // SMCMC_LIKE_EVENT_SAMPLE: the lanes' histograms, hist[bin][lane] (event_sample_loglike), in dynamic LDS
    double* es_hist = nullptr;
    if constexpr (LIKE == SMCMC_LIKE_EVENT_SAMPLE || LIKE == SMCMC_LIKE_EVENT_TEMPLATE || LIKE == SMCMC_LIKE_EVENT_SHAPE) {
        extern __shared__ __attribute__((aligned(16))) double es_dynamic[];
        es_hist = es_dynamic;
    }
    (void)es_hist;

    const int lane = SHARED ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;
    // SHARED: a wavefront past the last group (`live` false, wave-uniform) takes the last group's place in every address
    // it forms, so that all it reads exists; it is idle in every lane, runs no step and stores nothing
    const int ngroups = p.npad / kWave;
    const bool live = !SHARED || step_group_of((int)blockIdx.x, wave) < ngroups;
    const int group = !SHARED ? (int)blockIdx.x : live ? step_group_of((int)blockIdx.x, wave) : ngroups - 1;
    const int nsteps = live ? p.nsteps : 0;
    const int chain = group * kWave + lane;
    const bool active = live && chain < p.nchains;
    const int D = p.dim;
    const size_t NP = (size_t)p.npad;
    const uint32_t gid = p.chain_offset + (uint32_t)chain;
    const cptr_f64 c0 = as_const(p.c0);
    const cptr_f64 likep = as_const(p.like);
    double* const xcol = xs + XL::LANE * lane;   // this lane's column: row d at xcol[XL::row(d)]
    // PAIRS only (the other layouts go row by row, where they always did): the accepted point from the column into
    // registers / from registers into the column, a row pair per access
    auto load_point = [&](double (&dst)[DP]) {
#pragma unroll
        for (int q = 0; q < DP / 2; ++q) {
            const f64x2 v = *(const f64x2*)(xcol + XL::row(2 * q));
            dst[2 * q] = v[0];
            dst[2 * q + 1] = v[1];
        }
    };
    auto store_point = [&](const double (&src)[DP]) {
#pragma unroll
        for (int q = 0; q < DP / 2; ++q) {
            f64x2 v;
            v[0] = src[2 * q];
            v[1] = src[2 * q + 1];
            *(f64x2*)(xcol + XL::row(2 * q)) = v;
        }
    };
    (void)load_point;
    (void)store_point;

    // Lanes past the last chain hold x = c0 so that their y = x - c0 is +0 in the
    // moment contraction; they never accept and never store.
    if constexpr (PAIRS) {
        // (in pairs as well: an 8-byte write of a column that is 16 bytes from lane to lane is a two-way bank conflict)
        double xin[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) xin[d] = active ? p.x[(size_t)d * NP + chain] : c0[d];
        store_point(xin);
    } else {
#pragma unroll
        for (int d = 0; d < DP; ++d) xcol[XL::row(d)] = active ? p.x[(size_t)d * NP + chain] : c0[d];
    }

    double* lf = p.lane_f64 + chain;
    int32_t* li = p.lane_i32 + chain;
    double logl = lf[SMCMC_LANE_LOGL * NP];
    double sigma = lf[SMCMC_LANE_SIGMA * NP];
    double acc_rate = lf[SMCMC_LANE_ACCEPTANCE * NP];
    double acc_trials = lf[SMCMC_LANE_ACCEPTANCE_TRIALS * NP];
    double rigid = lf[SMCMC_LANE_RIGIDITY * NP];
    double last_value = lf[SMCMC_LANE_LAST_VALUE * NP];
    double last_x0 = lf[SMCMC_LANE_LAST_X0 * NP];
    double step_rms = lf[SMCMC_LANE_STEP_RMS * NP];
    double logl_prop = lf[SMCMC_LANE_LOGL_PROPOSED * NP];
    int trials = li[SMCMC_LANE_TRIALS * NP];
    int succ = li[SMCMC_LANE_SUCCESSES * NP];
    int next_update = li[SMCMC_LANE_NEXT_UPDATE * NP];
    int naccept = li[SMCMC_LANE_NACCEPT * NP];
    int rms_trials = li[SMCMC_LANE_STEP_RMS_TRIALS * NP];
    int last_accept = li[SMCMC_LANE_LAST_ACCEPT * NP];

    // stage U: lane-strided copy of each kept row segment
    const int tid = (int)threadIdx.x;   // (the staging is the workgroup's: SHARED, all its wavefronts')
#pragma unroll
    for (int i = 0; i < DP; ++i) {
        for (int k = tid; k < UL::len(i); k += NTHREADS) {
            const int j = UL::j0(i) + k;
            us[UL::off(i) + k] = (j < DP) ? p.U[i * DP + j] : 0.0;
        }
    }

    uint32_t ltab, atab;   // LDS byte addresses the gathers start from
    if constexpr (SHARED) {
        // slot s of a table (16 bytes at NormalTableLayout::slot_offset(s)) holds entry slot_entry(s) of the source
        typedef LogTableLayout LT;
        typedef AngleTableLayout AT;
        double* const atb = ntab + (WL::ANGLE - WL::LOG) / 8;
        for (int s = tid; s < LT::SLOTS; s += NTHREADS) {
            const int k = LT::slot_entry(s);
            f64x2 v;
            v[0] = smcmc_log_table_dev[2 * k];
            v[1] = smcmc_log_table_dev[2 * k + 1];
            *(f64x2*)(ntab + LT::slot_offset(s) / 8) = v;
        }
        for (int s = tid; s < AT::SLOTS; s += NTHREADS) {
            // entry 64 + k is entry k turned by pi / 2: (-sin, cos) (SMCMC_NORMAL_PAIR_BODY_HALFCIRCLE)
            const int e = AT::slot_entry(s), k = e & 63;
            const double c = smcmc_angle_table_dev[2 * k], sn = smcmc_angle_table_dev[2 * k + 1];
            f64x2 v;
            v[0] = (e < 64) ? c : -sn;
            v[1] = (e < 64) ? sn : c;
            *(f64x2*)(atb + AT::slot_offset(s) / 8) = v;
        }
        ltab = (uint32_t)(uintptr_t)(lds_cptr_f64)ntab + (uint32_t)LT::lane_offset(lane);
        atab = (uint32_t)(uintptr_t)(lds_cptr_f64)atb + (uint32_t)AT::lane_offset(lane);
    } else {
        for (int k = lane; k < 128; k += kWave) ntab[k] = smcmc_log_table_dev[k];
        for (int k = lane; k < 64; k += kWave) {
            // entry 64 + k is entry k turned by pi / 2: (-sin, cos) (SMCMC_NORMAL_PAIR_BODY_HALFCIRCLE)
            const double c = smcmc_angle_table_dev[2 * k], sn = smcmc_angle_table_dev[2 * k + 1];
            ntab[128 + 2 * k] = c;
            ntab[128 + 2 * k + 1] = sn;
            ntab[128 + 128 + 2 * k] = -sn;
            ntab[128 + 128 + 2 * k + 1] = c;
        }
        ltab = (uint32_t)(uintptr_t)(lds_cptr_f64)ntab;
        atab = ltab + 128u * 8u;
    }
    constexpr int LSH = SHARED ? LogTableLayout::SHIFT : 4, ASH = SHARED ? AngleTableLayout::SHIFT : 4;

    constexpr bool STRIP = MOMENTS && Geo<DP>::STRIP;
    constexpr int NT16 = Geo<DP>::NT16;
    f64x4 acc[MOMENTS ? NT16 : 1];
    double accs[STRIP ? T : 1];    // strip accumulators: (row 16 T16 + (lane >> 4), column 16 t + (lane & 15))
    double c0r[MOMENTS ? T : 1];   // c0 of the tile rows this lane feeds to the matrix pipe
    int xrow[MOMENTS ? T : 1];     // LDS row (clamped to the ones row) of those tile rows
    double c0s = 0.0;              // the same for the strip rows 16 T16 + (lane & 3)
    int xsrow = 0;
    if constexpr (MOMENTS) {
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[t][r] = p.gacc[(((size_t)group * NT + t) * 4 + r) * kWave + lane];
        if constexpr (STRIP) {
#pragma unroll
            for (int t = 0; t < T; ++t) accs[t] = p.gacc[(((size_t)group * NT + NT16 + t) * 4) * kWave + lane];
            const int r = 16 * Geo<DP>::T16 + (lane & 3);
            c0s = (r < DP) ? p.c0[r] : 0.0;
            xsrow = XL::row((r <= DP) ? r : (ZROW ? XL::ZERO_ROW : DP)) + XL::LANE * (lane >> 4);
        }
        // row DP carries the constant 1 (sum y and the point count come out of the
        // same contraction); tile rows above it are zero and are not stored
        // The rows the image holds above it -- in row pairs the ones row's partner -- are +0, in idle lanes too.  ZROW: the
        // operand reads of the tile rows past the ones row go there; otherwise no lane reads them (the operand reads clamp
        // to the ones row), but nothing in the image is left unwritten.  PAIRS: one 16-byte write.
        if constexpr (PAIRS) {
            static_assert(XL::HELD == DP + 2, "the ones row and its partner are one pair");
            f64x2 ones;
            ones[0] = active ? 1.0 : 0.0;
            ones[1] = 0.0;
            *(f64x2*)(xcol + XL::row(DP)) = ones;
        } else {
            xcol[XL::row(DP)] = active ? 1.0 : 0.0;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int r = 16 * t + (lane & 15);
            c0r[t] = (r < DP) ? p.c0[r] : 0.0;
            xrow[t] = XL::row((r <= DP) ? r : (ZROW ? XL::ZERO_ROW : DP)) + XL::LANE * (lane >> 4);
        }
    }
    __syncthreads();

    // operand prefetch of the fold (fetch_operands): only where a k-quad's matrix instructions span several pieces, only
    // with the other hand-placed reads (kAsmReads), only in the common kernels (triangular decomposition, no uniform
    // dimensions / scan) and not in the 63-dimension family: there the kernels are short of registers and the compiler
    // spilled the prefetched operands behind their reads in one variant or another (the build's listing check
    // refused them)
    constexpr bool OPF = MOMENTS && T >= 3 && kAsmReads<DP> && DP <= 50 && !FULLU && !SPECIAL;
    constexpr int KQ = 4 * 8 * XL::LANE;   // bytes from a k-quad's four lanes of the image to the next one's
    double raw[OPF ? T : 1], raws = 0.0;
    uint32_t xaddr[OPF ? T : 1], xsaddr = 0;
    if constexpr (OPF) {
#pragma unroll
        for (int t = 0; t < T; ++t) xaddr[t] = (uint32_t)(uintptr_t)(lds_cptr_f64)(xs + xrow[t]);
        if constexpr (STRIP) xsaddr = (uint32_t)(uintptr_t)(lds_cptr_f64)(xs + xsrow);
    }

    double xp[DP];
    const uint32_t aw = smcmc_accept_word((uint32_t)D);
#ifdef SMCMC_STEP_PROFILE
    StepProf prof;
    prof.start();
#endif

    // QUADFORM: the proposal and the accepted point trade places -- the likelihood reads the proposal from
    // the LDS column, the registers keep the accepted point to put back on a reject
    constexpr bool SWAP = (LIKE == SMCMC_LIKE_QUADFORM);

    // The step boundary without its waits (BOUNDARY; profiles/step_issue_notes.md): the StepRMS rows read in one batch,
    // coordinate 0 of the accepted point carried in a register, no wait for the commit's writes.  Only the instantiations
    // it was measured on have it: the headline's (D = 50 family, iso-Gaussian, reference order, triangular decomposition,
    // no uniform dimensions / scan; with and without the moment fold), whose lone wavefront per SIMD has the registers
    // for the 50 extra rows.  The fused-order and SPECIAL kernels of the family sit at 512 registers and spill already,
    // the families below 47 share a SIMD between two wavefronts, and the other likelihoods and the 47-dimension family
    // have no timing yet.  Every other instantiation keeps the step boundary it had, instruction for instruction.
    constexpr bool BOUNDARY = EXACT && !SWAP && !FULLU && !SPECIAL && DP == 50 && LIKE == SMCMC_LIKE_ISO_GAUSS;
    // ... and, with the moment fold, its matrix instructions dealt over the pieces by plan (smcmc_step_deal.h;
    // profiles/step_shadow_notes.md) instead of evenly by piece number
    constexpr bool DEAL = BOUNDARY && MOMENTS && OPF && Geo<DP>::STRIP;

    // Coordinate 0 of the accepted point, which UpdateState compares with the step before.  BOUNDARY: carried in a register
    // from commit to commit (read back from LDS at the top of a step it was a read and a full wait behind the commit's
    // writes); otherwise read at the top of every step.
    // With the moment fold (TOP_FREE) the read is final before the loop (the empty statement uses the value): left in
    // flight, the compiler's wait for it stood inside the loop, a full `s_waitcnt lgkmcnt(0)` at the top of every step,
    // right behind the commit's writes -- and the reload of the accepted point goes out at the top of the step (below).
    // The kernel without the fold measured 0.7 % slower with the two (profiles/step_boundary_notes.md) and keeps its top.
    constexpr bool TOP_FREE = BOUNDARY && MOMENTS;
    double x0 = 0.0;
    if constexpr (BOUNDARY && PAIRS) x0 = (*(const f64x2*)(xcol + XL::row(0)))[0];   // (the pair: no bank conflict)
    else if constexpr (BOUNDARY) x0 = xcol[XL::row(0)];
    if constexpr (TOP_FREE) asm volatile("" : "+v"(x0));

    // StepRMS window, likelihood, Metropolis test and accept copy of one step
    // (TSimpleMCMC.H:391-406, 410-491) for the proposal held in xp.
    auto finish_step = [&](int s, uint32_t uword) {
        if constexpr (SPECIAL || !EXACT) {
            // GetProposed() (TSimpleMCMC.H:514): the proposal of the latest step, accepted or not (in the reference
            // order only the SPECIAL instantiation carries the store; the fused kernels all do)
            if (p.proposed != nullptr && s + 1 == p.nsteps && active) {
#pragma unroll
                for (int d = 0; d < DP; ++d) p.proposed[(size_t)d * NP + chain] = xp[d];
            }
        }
        if constexpr (SWAP) {
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const double t = xcol[XL::row(d)];
                xcol[XL::row(d)] = xp[d];
                xp[d] = t;
            }
        }
        // The StepRMS sum needs the accepted point next to the proposal: DP rows of the LDS column.  Read where they
        // are used, every term is a read, a full wait and its arithmetic -- the LDS latency DP / 2 times per step, in a
        // lone wavefront that has nothing else to issue.  In the BOUNDARY kernels (the likelihood works on registers alone) the
        // rows are all read first, in one batch, and the terms wait with counted waits as the rows come in.  The likelihood
        // is written between the reads and the sum (two independent sums, each in its own order) so that it could run
        // under the reads; the compiler merges the two `step_rms_window > 0` blocks and puts it behind the sum in that
        // path, so one LDS latency is still exposed (profiles/step_issue_notes.md).
        // Taking the terms block by block inside the step instead (rows 4b .. 4b+3 of the proposal are final behind the
        // last piece of block b; two hand-placed row-pair reads per block under the block's last piece, no wait of their
        // own, no batch) was built and measured: the 17 waits of the batch go, but the ten registers the reads and the
        // running sum hold through the pieces push finished rows of the proposal into accumulation registers (55 - 130
        // more copies per step), and neither kernel gained beyond the runs' spread -- the one without the fold lost 1 %
        // (profiles/step_rms_blocks_notes.md).  The batch stays.
        constexpr bool RMS_AHEAD = BOUNDARY;
        double xold[RMS_AHEAD ? DP : 1];
        if constexpr (RMS_AHEAD) {
            if (p.step_rms_window > 0) {
                if constexpr (PAIRS) load_point(xold);
                else {
#pragma unroll
                    for (int d = 0; d < DP; ++d) xold[d] = xcol[XL::row(d)];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            logl_prop = loglike<DP, LIKE, EXACT>(xp, likep + p.zero * (s + 1), D);
            __builtin_amdgcn_sched_barrier(0);
            SMCMC_PROF_MARK(PROF_LIKE);
        }
        if (p.step_rms_window > 0) {
            double sqr = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                double t;
                if constexpr (RMS_AHEAD) t = xp[d] - xold[d];
                else t = SWAP ? xcol[XL::row(d)] - xp[d] : xp[d] - xcol[XL::row(d)];
                if constexpr (EXACT) sqr += t * t;
                else sqr = SMCMC_FMA(t, t, sqr);
            }
            double ms = step_rms * step_rms;
            ms *= rms_trials;
            ms += sqr;
            ms /= rms_trials + 1.0;
            rms_trials = (p.step_rms_window < rms_trials + 1) ? p.step_rms_window : rms_trials + 1;
            step_rms = __builtin_sqrt(ms);
        }
        SMCMC_PROF_MARK(PROF_RMS);
        if constexpr (SWAP) {
            bool dense = p.like_rowptr == nullptr;
            if (!dense) {
                const QuadCsr csr = {p.like_rowptr + p.zero * (s + 1), p.like_cols, p.like_vals, p.like_rows};
                logl_prop = quadform_csr<EXACT>([&](int j) { return xcol[XL::row(j)]; }, csr, D);
                dense = __any(!__builtin_isfinite(logl_prop));
            }
            if (dense) logl_prop = loglike_quadform_lds<DP, EXACT, XL>(xcol, likep + p.zero * (s + 1));
        }
        else if constexpr (LIKE == SMCMC_LIKE_EVENT_SAMPLE) logl_prop = event_sample_loglike<DP>(xp, likep + p.zero * (s + 1), es_hist, lane);
        else if constexpr (LIKE == SMCMC_LIKE_EVENT_TEMPLATE)
            logl_prop = event_two_pass_loglike<DP, false>(xp, likep + p.zero * (s + 1), es_hist, lane, p.like_park + chain, NP);
        else if constexpr (LIKE == SMCMC_LIKE_EVENT_SHAPE)
            logl_prop = event_two_pass_loglike<DP, true>(xp, likep + p.zero * (s + 1), es_hist, lane, p.like_park + chain, NP);
        else if constexpr (!RMS_AHEAD) logl_prop = loglike<DP, LIKE, EXACT>(xp, likep + p.zero * (s + 1), D);
        if constexpr (!RMS_AHEAD) SMCMC_PROF_MARK(PROF_LIKE);
        bool take;
        if (p.metropolis == 2) {
            take = true;
        } else if (!__builtin_isfinite(logl_prop) || logl_prop < -0.999999E+30) {
            take = false;
        } else {
            const double delta = logl_prop - logl;
            take = true;
            if (delta < 0.0) {
                if (p.metropolis == 1) take = false;
                else {
                    const double trial = smcmc_log_pos(smcmc_u01(uword));
                    if (delta < trial) take = false;
                }
            }
        }
        take = take && active;
        last_accept = take ? 1 : 0;
        if (take) {
            logl = logl_prop;
            ++naccept;
        }
        SMCMC_PROF_MARK(PROF_TEST);
        if (take != SWAP) {   // plain: commit the proposal on accept; swapped: put the accepted point back on reject
            if constexpr (PAIRS) store_point(xp);
            else {
#pragma unroll
                for (int d = 0; d < DP; ++d) xcol[XL::row(d)] = xp[d];
            }
        }
        SMCMC_PROF_MARK(PROF_COMMIT);
        if constexpr (BOUNDARY) x0 = take ? xp[0] : x0;
        // The next step's operand reads (inline assembly) must see this step's accepts.  The image is ONE wavefront's
        // (SHARED: its own among the workgroup's) and its LDS operations execute in issue order: all that is needed is that the compiler keeps the order, not a
        // barrier and not a wait for the writes -- they drain under the next step's scalar half.  The compiler keeps it
        // because this statement clobbers memory and because the operand reads (fetch_operands, fetch_operand) are
        // `asm volatile`, which are never reordered among each other: those reads must stay volatile.
        if constexpr (MOMENTS && BOUNDARY) asm volatile("" ::: "memory");
        else if constexpr (MOMENTS) __syncthreads();   // the next step's operand reads see this step's accepts
        SMCMC_PROF_MARK(PROF_ENDWAIT);
        if (p.save_x != nullptr && ((s + 1) % p.save_stride) == 0 && active) {
            const size_t slot = (size_t)((s + 1) / p.save_stride - 1);
#pragma unroll
            for (int d = 0; d < DP; ++d) p.save_x[(slot * (size_t)DP + (size_t)d) * NP + chain] = xcol[XL::row(d)];
            p.save_logl[slot * NP + chain] = logl;
        }
    };

    int s0 = 0;
    if (p.has_forced && nsteps > 0) {
        // ForceStep (TSimpleMCMC.H:671-678): the proposal is the forced point and the
        // proposal state is not updated
#pragma unroll
        for (int d = 0; d < DP; ++d) xp[d] = p.forced[(size_t)d * NP + chain];
        smcmc_u32x4 blk = smcmc_draw_block(p.seed, gid, (uint64_t)(p.step0 + 1u), aw >> 2, SMCMC_STREAM_STEP);
        finish_step(0, smcmc_select_word(blk, aw & 3u));
        s0 = 1;
    }

    if (SPECIAL && p.scan_dim >= 0) {
        // scan of one dimension (TSimpleMCMC.H:685-704): the proposal is the current point
        // with that dimension redrawn; the proposal state is not updated
        const uint32_t sd = (uint32_t)p.scan_dim;
#pragma nounroll
        for (int s = s0; s < nsteps; ++s) {
            const uint64_t step = (uint64_t)(p.step0 + (uint32_t)s + 1u);
            const smcmc_u32x4 sblk = smcmc_draw_block(p.seed, gid, step, sd >> 2, SMCMC_STREAM_STEP);
            double val;
            if (p.scan_uniform) {
                val = p.scan_a + (p.scan_b - p.scan_a) * smcmc_u01(smcmc_select_word(sblk, sd & 3u));
            } else {
                double nc, ns;
                smcmc_normal_pair(smcmc_select_word(sblk, sd & 2u), smcmc_select_word(sblk, (sd & 2u) + 1u), &nc, &ns);
                val = p.scan_a + p.scan_b * ((sd & 1u) ? ns : nc);
            }
#pragma unroll
            for (int d = 0; d < DP; ++d) xp[d] = ((uint32_t)d == sd) ? val : xcol[XL::row(d)];
            const smcmc_u32x4 ablk = smcmc_draw_block(p.seed, gid, step, aw >> 2, SMCMC_STREAM_STEP);
            finish_step(s, smcmc_select_word(ablk, aw & 3u));
        }
        s0 = nsteps;
    }

    for (int s = s0; s < nsteps; ++s) {
        const uint64_t step = (uint64_t)(p.step0 + (uint32_t)s + 1u);   // ++fTotalSteps, :376
        SMCMC_PROF_MARK(PROF_LOOP);
        SMCMC_PROF_MARK(PROF_STAMP);

        // TOP_FREE: the proposal starts from the accepted point, and its reload goes out here, in front of A: behind the
        // commit of the step before in program order (one wavefront, LDS operations execute in issue order), so that the
        // commit's writes and these reads are on their way under A's divisions and `pow`.  Issued behind A they came back
        // under nothing (the compiler does not lift them over A's branches).
        if constexpr (TOP_FREE && PAIRS) load_point(xp);
        else if constexpr (TOP_FREE) {
#pragma unroll
            for (int d = 0; d < DP; ++d) xp[d] = xcol[XL::row(d)];
        }

        // ---- A: UpdateState, scalar half (TSimpleMCMC.H:1723-1776) ----
        ++trials;
        if constexpr (!BOUNDARY) x0 = xcol[XL::row(0)];
        const bool moved = (logl != last_value) || (x0 != last_x0);
        if (moved) ++succ;
        acc_rate *= acc_trials;
        if (moved) acc_rate = acc_rate + 1.0;
        acc_rate /= acc_trials + 1.0;
        acc_trials = dmin(p.acc_window, acc_trials + 1.0);
        if (rigid < 500.0 && rigid > 0.0) {
            if (__builtin_fabs(acc_rate - p.target) < p.asig) {
                rigid += 0.5 * rigid / p.acc_window;
                rigid = dmin(200.0, rigid);
            }
            if (__builtin_fabs(acc_rate - p.target) > 4.0 * p.asig) {
                rigid -= 1.618 * 0.5 * rigid / p.acc_window;
                rigid = dmax(2.0, rigid);
            }
        }
        if (rigid > 0 && rigid < 100.0) {
            sigma *= smcmc_pow_small(acc_rate / p.target,
                                     dmin(1.0 / 500.0, 1.0 / (rigid * p.acc_window)));
        }
        if constexpr (!MOMENTS) {
            if (p.per_lane_update && moved && (--next_update) < 1) {
                // per-chain UpdateProposal on a frozen covariance (TSimpleMCMC.H:1824-1826,
                // 1050-1052, 1081-1086); trace unchanged => sigma and U unchanged
                double up = 0.5 * succ;
                next_update = (int)(p.acc_window + p.max_up - p.max_up / (up + 1.0));
                if (p.acc_w >= 0.0) {
                    acc_trials = dmax(1.0, p.acc_w * acc_trials);
                    acc_trials = dmin(acc_trials, p.acc_wW);
                }
            }
        }
        last_value = logl;
        last_x0 = x0;
        SMCMC_PROF_MARK(PROF_A);

        // ---- B: proposal (TSimpleMCMC.H:709-724) ----
        if constexpr (OPF) {
            fetch_operands<T, 0, KQ>(xaddr, raw);
            if constexpr (STRIP) fetch_operand<0, KQ>(xsaddr, raws);
        }
        if constexpr (!TOP_FREE && PAIRS) load_point(xp);
        else if constexpr (!TOP_FREE) {
#pragma unroll
            for (int d = 0; d < DP; ++d) xp[d] = xcol[XL::row(d)];
        }
        uint32_t uword = 0;
        // The LDS image of U never changes, so the compiler would hoist all of its reads out
        // of the step loop and spill them; reading through a pointer it cannot see through
        // keeps them inside the step.
        uint32_t up = (uint32_t)(uintptr_t)(lds_cptr_f64)us;   // LDS byte address of the decomposition
        asm volatile("" : "+v"(up));
        double ma[MOMENTS ? T : 1];   // matrix-pipe operands of the chain quad being folded
        double ms = 0.0;              // ... and the strip rows' operand
        // The Philox block and the table entries of the NEXT block of four normals are made during the last piece of the
        // current one (kAsmReads: the table reads then have a whole piece to come back in, and sit in the registers the
        // idle `nxt` buffer leaves free); two sets in turn, indexed at compile time -- never copied while in flight.
        constexpr bool PIPE = kAsmReads<DP>;
        smcmc_u32x4 blks[2];
        NormalTables tabs[2][2];
        auto draw_and_fetch = [&](auto bn) {
            constexpr int b1 = decltype(bn)::value;
            blks[b1 & 1] = smcmc_draw_block(p.seed, gid, step, (uint32_t)b1, SMCMC_STREAM_STEP);
            tabs[b1 & 1][0] = normal_tables_fetch<kAsmReads<DP>, LSH, ASH>(blks[b1 & 1].v[0], blks[b1 & 1].v[1], ltab, atab);
            if constexpr (4 * b1 + 2 < DP)
                tabs[b1 & 1][1] = normal_tables_fetch<kAsmReads<DP>, LSH, ASH>(blks[b1 & 1].v[2], blks[b1 & 1].v[3], ltab, atab);
        };
        if constexpr (PIPE) draw_and_fetch(std::integral_constant<int, 0>{});
        SMCMC_PROF_MARK(PROF_TOP);
        static_for<NB>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            // U rows 4b..4b+3 are consumed in pieces of kPiece columns; the LDS reads of a
            // piece are issued one piece ahead of its use (the first one before the random
            // numbers are made), and each piece is its own scheduling region: the scheduler
            // otherwise issues every read of the step up front and spills hundreds of registers.
            typedef UPieces<DP, FULLU, b> PC;
            f64x2 cur[kPiece / 2], nxt[kPiece / 2];

            if constexpr (!PIPE) draw_and_fetch(bc);
            smcmc_u32x4& blk = blks[b & 1];
            // FIXED_AW: the accept word lies in block AcceptBlock<DP>::BLOCK for every dimension this kernel is launched at
            if constexpr (FIXED_AW) {
                if constexpr (b == AcceptBlock<DP>::BLOCK) uword = smcmc_select_word(blk, aw & 3u);
            } else if ((uint32_t)b == (aw >> 2)) uword = smcmc_select_word(blk, aw & 3u);
            // LDS reads of the block, in this order (they return in issue order): the table entries of its two pairs of
            // normals (issued here, or during the last piece of the block before), then the first piece of U, which
            // stays in flight under the normals' arithmetic
            NormalTables& t0 = tabs[b & 1][0];
            NormalTables& t1 = tabs[b & 1][1];
            {
                constexpr int i0 = PC::row(0), c0p = PC::col(0);
                load_piece<DP, FULLU, i0, c0p>(up, cur);
                if constexpr (4 * b + 2 < DP) normal_tables_ready<piece_reads<DP, FULLU, c0p>(), kAsmReads<DP>>(t0, t1);
                else normal_tables_ready<piece_reads<DP, FULLU, c0p>(), kAsmReads<DP>>(t0);
                // the reads stay right behind the matrix instruction that closed the block before: the vector
                // instructions of the normals that need no table would otherwise go first, and wait for it
                if constexpr (DEAL) __builtin_amdgcn_sched_barrier(0);
            }
            double n[4];
            normal_pair_lds(blk.v[0], blk.v[1], t0, &n[0], &n[1]);
            if constexpr (4 * b + 2 < DP) normal_pair_lds(blk.v[2], blk.v[3], t1, &n[2], &n[3]);
            else { n[2] = 0.0; n[3] = 0.0; }
            double sr[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) sr[q] = sigma * n[q];
            __builtin_amdgcn_sched_barrier(0);
            SMCMC_PROF_MARK(PROF_NORMALS);

            static_for<PC::COUNT>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                constexpr int i = PC::row(r), c = PC::col(r);
                constexpr int g = PC::first_global() + r;          // piece number within the step
                (void)g;
                if constexpr (r + 1 < PC::COUNT) {
                    constexpr int i1 = PC::row(r + 1), c1 = PC::col(r + 1);
                    load_piece<DP, FULLU, i1, c1>(up, nxt);
                    piece_ready<piece_reads<DP, FULLU, c1>(), piece_reads<DP, FULLU, c>(), kAsmReads<DP>>(cur);
                    SMCMC_PROF_PIECE(PROF_PIECE_DRAIN, g);
                } else {
                    piece_ready<0, piece_reads<DP, FULLU, c>(), kAsmReads<DP>>(cur);
                    SMCMC_PROF_PIECE(PROF_PIECE_DRAIN, g);
                    // the last piece of the block: the next block's random words and its table reads
                    if constexpr (PIPE && b + 1 < NB) draw_and_fetch(std::integral_constant<int, b + 1>{});
                }
                const double srow = sr[i - 4 * b];
#pragma unroll
                for (int k = 0; k < kPiece; ++k) {
                    const int j = c + k;
                    if (j < DP && (FULLU || j >= i)) {
                        const double u = cur[k / 2][k & 1];
                        if constexpr (EXACT) xp[j] += srow * u;
                        else xp[j] = SMCMC_FMA(srow, u, xp[j]);
                        // pins this update between the (ordered) LDS reads around it; without it
                        // the arithmetic of the whole step sinks below all the reads, which then
                        // have to be spilled
                        asm volatile("" : "+v"(xp[j]));
                    }
                }
                SMCMC_PROF_PIECE(PROF_PIECE_VALU, g);
                if constexpr (MOMENTS) {
                    // The group's second moments: the 16 x NT matrix instructions of the 64-chain contraction are
                    // dealt out over the pieces of the step (1-2 per piece) and pinned BEHIND the piece's vector work.
                    // An FP64 matrix instruction holds the vector pipe for its 64 cycles but not the issue of LDS
                    // reads, waits and scalar instructions: what follows it here is exactly that -- the prefetched
                    // operands of the next k-quad, then the next piece's eight reads and its wait -- and runs in
                    // its shadow.  (Left to the scheduler it goes to the top of the piece, in front of 32 vector
                    // instructions that then wait for it.)  Chains fold in ascending order.
                    if constexpr (DEAL) {
                        // The headline kernels deal by the plan of smcmc_step_deal.h instead of by piece number: one
                        // 16x16 per slot, last in its slot (what follows the slot issues in ITS shadow), the strip
                        // instructions in front of it or alone behind the pieces whose successor has few reads, the
                        // operand prefetch at the end of the slot that opens a k-quad.  The order inside a slot is pinned
                        // (left alone the scheduler puts a strip instruction behind the 16x16), and so is the operand
                        // preparation in front of the k-quad's first instruction (left alone, all but the first operand's
                        // sink behind it and wait out its 64 cycles).
                        static_assert(StepDeal<DP>::valid(kStepDealPlan<DP>) && StepDeal<DP>::G == UPieces<DP, FULLU, NB - 1>::first_global() + UPieces<DP, FULLU, NB - 1>::COUNT,
                                      "the plan keeps the operands' order: see smcmc_step_deal.h");
                        constexpr int m_lo = kStepDealPlan<DP>.first[g], m_hi = kStepDealPlan<DP>.first[g + 1];
                        if constexpr (m_hi > m_lo) __builtin_amdgcn_sched_barrier(0);
                        static_for<m_hi - m_lo>([&](auto mc) {
                            constexpr int m = m_lo + decltype(mc)::value;
                            constexpr int kk = kStepDealPlan<DP>.kk[m], tile = kStepDealPlan<DP>.tile[m];
                            if constexpr (m % NT == 0) {
                                operands_ready<T>(raw, raws);   // fetched a k-quad ago, a piece_ready since
#pragma unroll
                                for (int t = 0; t < T; ++t) {
                                    ma[t] = raw[t] - c0r[t];
                                    // rows past the ones row (ZROW: they read the zero row and c0r is 0 there: +0 as it stands)
                                    if (!ZROW && 16 * t + 15 > DP) ma[t] = (16 * t + (lane & 15) <= DP) ? ma[t] : 0.0;
                                }
                                ms = raws - c0s;
                                if constexpr (!ZROW) ms = (16 * Geo<DP>::T16 + (lane & 3) <= DP) ? ms : 0.0;
                                __builtin_amdgcn_sched_barrier(0);
                            }
                            if constexpr (tile < NT16) {
                                constexpr int ti = tile_row(tile), tj = tile - ti * (ti + 1) / 2;
                                acc[tile] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma[ti], ma[tj], acc[tile], 0, 0, 0);
                                asm volatile("" : "+a"(acc[tile]));   // keeps the instruction in this piece
                            } else {
                                constexpr int t = tile - NT16;
                                accs[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(ms, ma[t], accs[t], 0, 0, 0);
                                asm volatile("" : "+a"(accs[t]));
                            }
                            if constexpr (m + 1 < m_hi) __builtin_amdgcn_sched_barrier(0);
                            if constexpr (kStepDealPlan<DP>.pf_after[m]) {
                                fetch_operands<T, kk + 1, KQ>(xaddr, raw);
                                fetch_operand<kk + 1, KQ>(xsaddr, raws);
                            }
                        });
                    } else {
                        constexpr int G = UPieces<DP, FULLU, NB - 1>::first_global() + UPieces<DP, FULLU, NB - 1>::COUNT;
                        constexpr int NM = 16 * NT;
                        constexpr int m_lo = (int)(((long)g * NM) / G), m_hi = (int)(((long)(g + 1) * NM) / G);
                        if constexpr (m_hi > m_lo) __builtin_amdgcn_sched_barrier(0);
                        static_for<m_hi - m_lo>([&](auto mc) {
                            constexpr int m = m_lo + decltype(mc)::value;
                            constexpr int kk = m / NT, tile = m % NT;
                            if constexpr (tile == 0) {
                                if constexpr (OPF) operands_ready<T>(raw, raws);   // fetched a k-quad ago, a piece_ready since
#pragma unroll
                                for (int t = 0; t < T; ++t) {
                                    if constexpr (OPF) ma[t] = raw[t] - c0r[t];
                                    else ma[t] = xs[xrow[t] + 4 * XL::LANE * kk] - c0r[t];
                                    if (16 * t + 15 > DP) ma[t] = (16 * t + (lane & 15) <= DP) ? ma[t] : 0.0;   // rows past the ones row
                                }
                                if constexpr (STRIP) {
                                    if constexpr (OPF) ms = raws - c0s;
                                    else ms = xs[xsrow + 4 * XL::LANE * kk] - c0s;
                                    ms = (16 * Geo<DP>::T16 + (lane & 3) <= DP) ? ms : 0.0;
                                }
                            }
                            if constexpr (!STRIP || tile < NT16) {
                                constexpr int ti = tile_row(tile), tj = tile - ti * (ti + 1) / 2;
                                acc[tile] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma[ti], ma[tj], acc[tile], 0, 0, 0);
                                asm volatile("" : "+a"(acc[tile]));   // keeps the instruction in this piece
                            } else {
                                // A: strip rows (lane & 3) x chains (lane >> 4), the same for the four blocks;
                                // B: the column operand of tile column t, block (lane >> 2) & 3
                                constexpr int t = tile - NT16;
                                accs[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(ms, ma[t], accs[t], 0, 0, 0);
                                asm volatile("" : "+a"(accs[t]));
                            }
                            if constexpr (tile == 0 && OPF && kk + 1 < 16) {
                                // (behind the k-quad's first matrix instruction: in its shadow) the next k-quad's first
                                // matrix instruction sits in a later piece
                                static_assert(((long)(kk + 1) * NT * G) / NM > g, "operand prefetch needs a piece boundary");
                                fetch_operands<T, kk + 1, KQ>(xaddr, raw);
                                if constexpr (STRIP) fetch_operand<kk + 1, KQ>(xsaddr, raws);
                            }
                        });
                    }
                }
                SMCMC_PROF_PIECE(PROF_PIECE_MATRIX, g);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (r + 1 < PC::COUNT) {
#pragma unroll
                    for (int k = 0; k < kPiece / 2; ++k) cur[k] = nxt[k];
                }
            });
            SMCMC_PROF_MARK(PROF_PIECES);
        });
        // an accept word behind the blocks the proposal drew (never with FIXED_AW: its block is one of them)
        if (!FIXED_AW && (aw >> 2) >= (uint32_t)NB) {
            smcmc_u32x4 blk = smcmc_draw_block(p.seed, gid, step, aw >> 2, SMCMC_STREAM_STEP);
            uword = smcmc_select_word(blk, aw & 3u);
        }
        if (SPECIAL && p.uniform_mask != 0) {
            // uniform dimensions (TSimpleMCMC.H:711-716): word d of the step makes the draw; their
            // rows and columns of the device copy of U are zero, so nothing else touched them
            const cptr_f64 ub = as_const(p.uniform);
            uint64_t m = p.uniform_mask;
#pragma nounroll
            while (m != 0) {
                const uint32_t ud = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                const smcmc_u32x4 ublk = smcmc_draw_block(p.seed, gid, step, ud >> 2, SMCMC_STREAM_STEP);
                const double lo = ub[ud], hi = ub[DP + ud];
                const double val = lo + (hi - lo) * smcmc_u01(smcmc_select_word(ublk, ud & 3u));
#pragma unroll
                for (int d = 0; d < DP; ++d) xp[d] = ((uint32_t)d == ud) ? val : xp[d];
            }
        }
        SMCMC_PROF_MARK(PROF_TAIL);
        finish_step(s, uword);
    }

#ifdef SMCMC_STEP_PROFILE
    if (p.prof != nullptr) {
#pragma unroll
        for (int q = 0; q < kProfSlots; ++q) p.prof[((size_t)group * kProfSlots + q) * kWave + lane] += prof.slot[q];
    }
#endif
    if constexpr (MOMENTS) {
        if (live) {
#pragma unroll
            for (int t = 0; t < NT16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    p.gacc[(((size_t)group * NT + t) * 4 + r) * kWave + lane] = acc[t][r];
            if constexpr (STRIP) {
#pragma unroll
                for (int t = 0; t < T; ++t) p.gacc[(((size_t)group * NT + NT16 + t) * 4) * kWave + lane] = accs[t];
            }
        }
    }
    if (active) {
#pragma unroll
        for (int d = 0; d < DP; ++d) p.x[(size_t)d * NP + chain] = xcol[XL::row(d)];
        lf[SMCMC_LANE_LOGL * NP] = logl;
        lf[SMCMC_LANE_SIGMA * NP] = sigma;
        lf[SMCMC_LANE_ACCEPTANCE * NP] = acc_rate;
        lf[SMCMC_LANE_ACCEPTANCE_TRIALS * NP] = acc_trials;
        lf[SMCMC_LANE_RIGIDITY * NP] = rigid;
        lf[SMCMC_LANE_LAST_VALUE * NP] = last_value;
        lf[SMCMC_LANE_LAST_X0 * NP] = last_x0;
        lf[SMCMC_LANE_STEP_RMS * NP] = step_rms;
        lf[SMCMC_LANE_LOGL_PROPOSED * NP] = logl_prop;
        li[SMCMC_LANE_TRIALS * NP] = trials;
        li[SMCMC_LANE_SUCCESSES * NP] = succ;
        li[SMCMC_LANE_NEXT_UPDATE * NP] = next_update;
        li[SMCMC_LANE_NACCEPT * NP] = naccept;
        li[SMCMC_LANE_STEP_RMS_TRIALS * NP] = rms_trials;
        li[SMCMC_LANE_LAST_ACCEPT * NP] = last_accept;
    }
}

// Moment reduction, two ordered levels (the order is part of the engine's definition and
// is mirrored by oracle/ensemble_oracle.c): groups are summed in ascending order within
// chunks of kReduceChunk groups, then the chunk sums in ascending order.
constexpr int kReduceChunk = 32;

// offset of packed element k = (i, j), j <= i <= D, inside one group's tiles
template <int DP>
__device__ __forceinline__ size_t packed_to_tile_offset(int k, int D) {
    int i = (int)((__builtin_sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= k) ++i;
    while (i * (i + 1) / 2 > k) --i;
    const int j = k - i * (i + 1) / 2;
    const int ri = (i == D) ? DP : i, rj = (j == D) ? DP : j;   // the ones row sits at row DP of the tiles
    const int ti = ri >> 4, tj = rj >> 4, ii = ri & 15, jj = rj & 15;
    // C/D layout of v_mfma_f64_16x16x4_f64: column = lane & 15, row = (lane >> 4) + 4*reg
    const int reg = ii >> 2;
    const int lane = jj + 16 * (ii & 3);
    return ((size_t)(ti * (ti + 1) / 2 + tj) * 4 + reg) * kWave + lane;
}

// level 1: thread (k, chunk) -> chunk_sums[chunk][k]; it leaves ZERO in the accumulator entries it read (the next window
// accumulates into them -- rounds 1-3 cleared all 21 MB of accumulators with a memset per window; entries nobody reads,
// the lower halves of the diagonal tiles, keep growing unread).
// (Both levels in one launch -- the last workgroup of a range of k adding the chunk sums -- was built and measured:
// 36 us instead of 14.  Workgroups on different XCDs only see each other's stores after an agent-scope release, which
// on this chip writes the XCD's L2 back, once per workgroup.)
template <int DP>
__global__ void reduce_chunks_kernel(double* __restrict__ gacc, int ngroups, int D, double* __restrict__ chunk_sums) {
    constexpr int NT = Geo<DP>::NT;
    const int npk = (D + 1) * (D + 2) / 2;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int chunk = blockIdx.y;
    if (k >= npk) return;
    const size_t off = packed_to_tile_offset<DP>(k, D);
    const size_t gstride = (size_t)NT * 4 * kWave;
    const int g0 = chunk * kReduceChunk;
    const int g1 = (g0 + kReduceChunk < ngroups) ? g0 + kReduceChunk : ngroups;
    double v[kReduceChunk];
#pragma unroll
    for (int q = 0; q < kReduceChunk; ++q) v[q] = (g0 + q < g1) ? gacc[(size_t)(g0 + q) * gstride + off] : 0.0;
#pragma unroll
    for (int q = 0; q < kReduceChunk; ++q)
        if (g0 + q < g1) gacc[(size_t)(g0 + q) * gstride + off] = 0.0;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kReduceChunk; ++q)
        if (g0 + q < g1) s += v[q];
    chunk_sums[(size_t)chunk * npk + k] = s;
}

// level 2: thread k -> moments[k]
template <int DP>
__global__ void reduce_final_kernel(const double* __restrict__ chunk_sums, int nchunks, int npk,
                                    double* __restrict__ moments) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npk) return;
    // (the loads go out in batches of 16 -- one at a time this launch was 9 us of load latency --, the additions stay in
    // chunk order)
    double s = 0.0;
    for (int c0 = 0; c0 < nchunks; c0 += 16) {
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = (c0 + q < nchunks) ? chunk_sums[(size_t)(c0 + q) * npk + k] : 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (c0 + q < nchunks) s += v[q];
    }
    moments[k] = s;
}

// Host-callable launchers, one translation unit per (DP, likelihood) (smcmc_inst.hip).
template <int DP, int LIKE> hipError_t launch_step_like(const StepParams& p, bool exact, bool fullu, bool moments,
                                                        bool special, hipStream_t stream);
template <int DP> hipError_t launch_reduce(double* gacc, int ngroups, int D, double* chunk_sums, double* moments,
                                           hipStream_t stream);

template <int DP>
inline hipError_t launch_step(const StepParams& p, int like, bool exact, bool fullu, bool moments, bool special,
                              hipStream_t stream) {
    switch (like) {
        case SMCMC_LIKE_ISO_GAUSS: return launch_step_like<DP, SMCMC_LIKE_ISO_GAUSS>(p, exact, fullu, moments, special, stream);
        case SMCMC_LIKE_QUADFORM: return launch_step_like<DP, SMCMC_LIKE_QUADFORM>(p, exact, fullu, moments, special, stream);
        case SMCMC_LIKE_ROSENBROCK: return launch_step_like<DP, SMCMC_LIKE_ROSENBROCK>(p, exact, fullu, moments, special, stream);
        // the stress likelihoods are built for two register-array sizes only (kStressDP)
        case SMCMC_LIKE_ASYM:
            if constexpr (DP == 31 || DP == 63) return launch_step_like<DP, SMCMC_LIKE_ASYM>(p, exact, fullu, moments, special, stream);
            else return hipErrorInvalidValue;
        case SMCMC_LIKE_HORRIFIC:
            if constexpr (DP == 31 || DP == 63) return launch_step_like<DP, SMCMC_LIKE_HORRIFIC>(p, exact, fullu, moments, special, stream);
            else return hipErrorInvalidValue;
        case SMCMC_LIKE_CONSTRAINED:
            if constexpr (DP == 31 || DP == 63) return launch_step_like<DP, SMCMC_LIKE_CONSTRAINED>(p, exact, fullu, moments, special, stream);
            else return hipErrorInvalidValue;
        // the event sample and the event template are built for the family of their nine dimensions only (kEsDP)
        case SMCMC_LIKE_EVENT_SAMPLE:
            if constexpr (DP == kEsDP) return launch_step_like<DP, SMCMC_LIKE_EVENT_SAMPLE>(p, exact, fullu, moments, special, stream);
            else return hipErrorInvalidValue;
        case SMCMC_LIKE_EVENT_TEMPLATE:
            if constexpr (DP == kEsDP) return launch_step_like<DP, SMCMC_LIKE_EVENT_TEMPLATE>(p, exact, fullu, moments, special, stream);
            else return hipErrorInvalidValue;
        // ... and the event shape for the family of its 31 (kEshDP)
        case SMCMC_LIKE_EVENT_SHAPE:
            if constexpr (DP == kEshDP) return launch_step_like<DP, SMCMC_LIKE_EVENT_SHAPE>(p, exact, fullu, moments, special, stream);
            else return hipErrorInvalidValue;
#ifdef SMCMC_USER_LIKELIHOOD
        case SMCMC_LIKE_USER: return launch_step_like<DP, SMCMC_LIKE_USER>(p, exact, fullu, moments, special, stream);
#endif
        default: return hipErrorInvalidValue;
    }
}

}  // namespace smcmc
