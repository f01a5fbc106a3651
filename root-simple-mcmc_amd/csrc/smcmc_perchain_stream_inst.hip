// smcmc_perchain_stream_inst.hip -- instantiations of the one-chain-per-workgroup adaptive step with streamed matrices
// (smcmc_perchain_stream.hip.h): one kernel per likelihood, the dimension is a run-time value.
#include "smcmc_perchain_stream.hip.h"

namespace smcmc {

template <int LIKE>
static hipError_t go_stream(const PerChainParams& p, const PerChainRecord& rec, const PerChainStreamWork& w, hipStream_t s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(perchain_stream_kernel<LIKE>), dim3(p.nchains), dim3(kWgThreads), 0, s, p, rec, w);
    return hipGetLastError();
}

hipError_t launch_perchain_stream(const PerChainParams& p, const PerChainRecord& rec, const PerChainStreamWork& w, int like,
                                  hipStream_t s) {
    // operand shapes the kernel's indexing assumes
    if (p.dim < kStMinDim || p.dim > kStMaxDim || p.npad < kWave || p.npad % kWave != 0 || p.nchains < 1 || p.nchains > p.npad)
        return hipErrorInvalidValue;
    if (!p.x || !p.proposed || !p.last_point || !p.centre || !p.cov || !p.ut || !p.lane_f64 || !p.lane_i32 || !p.flag_count)
        return hipErrorInvalidValue;
    if (!w.wcov || !w.wu) return hipErrorInvalidValue;
    if (p.save_x && p.save_stride < 1) return hipErrorInvalidValue;
    if (rec.rec && (rec.chain < 0 || rec.chain >= p.nchains || rec.stride < 3 * p.dim + kPcRecScalars)) return hipErrorInvalidValue;
    switch (like) {
        case SMCMC_LIKE_ISO_GAUSS: return go_stream<SMCMC_LIKE_ISO_GAUSS>(p, rec, w, s);
        case SMCMC_LIKE_QUADFORM: return go_stream<SMCMC_LIKE_QUADFORM>(p, rec, w, s);
        case SMCMC_LIKE_ROSENBROCK: return go_stream<SMCMC_LIKE_ROSENBROCK>(p, rec, w, s);
        case SMCMC_LIKE_ASYM: return go_stream<SMCMC_LIKE_ASYM>(p, rec, w, s);
        case SMCMC_LIKE_HORRIFIC: return go_stream<SMCMC_LIKE_HORRIFIC>(p, rec, w, s);
        case SMCMC_LIKE_CONSTRAINED: return go_stream<SMCMC_LIKE_CONSTRAINED>(p, rec, w, s);
#if defined(SMCMC_USER_LIKELIHOOD) && defined(SMCMC_USER_LIKELIHOOD_ANY_DIM)
        case SMCMC_LIKE_USER: return go_stream<SMCMC_LIKE_USER>(p, rec, w, s);
#endif
        default: return hipErrorInvalidValue;
    }
}

}  // namespace smcmc
