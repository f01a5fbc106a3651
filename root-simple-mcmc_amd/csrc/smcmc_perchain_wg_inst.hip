// smcmc_perchain_wg_inst.hip -- instantiations of the one-chain-per-workgroup adaptive step
// (smcmc_perchain_wg.hip.h): likelihood x registers of packed covariance per thread.
#include "smcmc_perchain_wg.hip.h"

namespace smcmc {

template <int LIKE, int NE>
static hipError_t go_wg(const PerChainParams& p, const PerChainRecord& rec, hipStream_t s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(perchain_wg_kernel<LIKE, NE>), dim3(p.nchains), dim3(kWgThreads), 0, s, p, rec);
    return hipGetLastError();
}

template <int LIKE>
static hipError_t go_wg_like(const PerChainParams& p, const PerChainRecord& rec, hipStream_t s) {
    switch (perchain_wg_elements(p.dim)) {
        case 8: return go_wg<LIKE, 8>(p, rec, s);
        case 16: return go_wg<LIKE, 16>(p, rec, s);
        case kWgMaxNE: return go_wg<LIKE, kWgMaxNE>(p, rec, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_perchain_wg(const PerChainParams& p, const PerChainRecord& rec, int like, hipStream_t s) {
    // operand shapes the kernel's indexing assumes
    if (p.dim < 1 || p.dim > kWgMaxDim || p.npad < kWave || p.npad % kWave != 0 || p.nchains < 1 || p.nchains > p.npad)
        return hipErrorInvalidValue;
    if (!p.x || !p.proposed || !p.last_point || !p.centre || !p.cov || !p.ut || !p.lane_f64 || !p.lane_i32 || !p.flag_count)
        return hipErrorInvalidValue;
    if (p.save_x && p.save_stride < 1) return hipErrorInvalidValue;
    if (rec.rec && (rec.chain < 0 || rec.chain >= p.nchains || rec.stride < 3 * p.dim + kPcRecScalars)) return hipErrorInvalidValue;
    switch (like) {
        case SMCMC_LIKE_ISO_GAUSS: return go_wg_like<SMCMC_LIKE_ISO_GAUSS>(p, rec, s);
        case SMCMC_LIKE_QUADFORM: return go_wg_like<SMCMC_LIKE_QUADFORM>(p, rec, s);
        case SMCMC_LIKE_ROSENBROCK: return go_wg_like<SMCMC_LIKE_ROSENBROCK>(p, rec, s);
        case SMCMC_LIKE_ASYM: return go_wg_like<SMCMC_LIKE_ASYM>(p, rec, s);
        case SMCMC_LIKE_HORRIFIC: return go_wg_like<SMCMC_LIKE_HORRIFIC>(p, rec, s);
        case SMCMC_LIKE_CONSTRAINED: return go_wg_like<SMCMC_LIKE_CONSTRAINED>(p, rec, s);
#if defined(SMCMC_USER_LIKELIHOOD) && defined(SMCMC_USER_LIKELIHOOD_ANY_DIM)
        case SMCMC_LIKE_USER: return go_wg_like<SMCMC_LIKE_USER>(p, rec, s);
#endif
        default: return hipErrorInvalidValue;
    }
}

}  // namespace smcmc
