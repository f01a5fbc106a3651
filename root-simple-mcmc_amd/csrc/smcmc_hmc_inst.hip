// smcmc_hmc_inst.hip -- instantiations of the HMC step kernel for one workgroup shape;
// built once per -DSMCMC_PANEL_W=<wavefronts per chain group>.
#include "smcmc_hmc_kernel.hip.h"

#ifndef SMCMC_PANEL_W
#error "compile with -DSMCMC_PANEL_W=<4|8>"
#endif

namespace smcmc {

template <int W, int CW, int LIKE>
static hipError_t go_hmc(const HmcParams& p, hipStream_t s, const HmcSaveArgs* sv) {
    const HmcSaveArgs none = {nullptr, nullptr, 1, 0};
    // PotentialGradient types 2 / 3 / 5 (TSimpleHMC.H:467-532) live in the GENERIC instantiation
    const bool generic = p.gradient_type == 2 || p.gradient_type == 3 || p.gradient_type == 5;
    if (generic) {
        if (p.gradient_type == 2 && (p.cov_Eperm == nullptr || p.cov_average == nullptr)) return hipErrorInvalidValue;
        if (p.gradient_type == 3 && p.fd_grad == nullptr) return hipErrorInvalidValue;
        if (sv != nullptr) return hipErrorInvalidValue;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_step_kernel<W, CW, LIKE, true>), dim3(p.npad / kWave), dim3(W * kWave), 0, s, p, none);
    } else if (sv != nullptr) {
        if (sv->x == nullptr || sv->stride < 1 || sv->first < 0) return hipErrorInvalidValue;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_step_kernel<W, CW, LIKE, false, true>), dim3(p.npad / kWave), dim3(W * kWave), 0, s, p, *sv);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_step_kernel<W, CW, LIKE, false>), dim3(p.npad / kWave), dim3(W * kWave), 0, s, p, none);
    }
    return hipGetLastError();
}

// the likelihoods without a gradient of their own: the GENERIC instantiation only (Start's potential included)
template <int W, int CW, int LIKE>
static hipError_t go_hmc_no_gradient(const HmcParams& p, hipStream_t s, const HmcSaveArgs* sv) {
    if (sv != nullptr) return hipErrorInvalidValue;
    const HmcSaveArgs none = {nullptr, nullptr, 1, 0};
    if (!p.init_only) {
        if (!(p.gradient_type == 2 || p.gradient_type == 3 || p.gradient_type == 5)) return hipErrorInvalidValue;
        if (p.gradient_type == 2 && (p.cov_Eperm == nullptr || p.cov_average == nullptr)) return hipErrorInvalidValue;
        if (p.gradient_type == 3 && p.fd_grad == nullptr) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_step_kernel<W, CW, LIKE, true>), dim3(p.npad / kWave), dim3(W * kWave), 0, s, p, none);
    return hipGetLastError();
}

template <>
hipError_t launch_hmc<SMCMC_PANEL_W, kPanelCW>(const HmcParams& p, int like, hipStream_t s, const HmcSaveArgs* sv) {
    constexpr int W = SMCMC_PANEL_W, CW = kPanelCW;
    switch (like) {
        case SMCMC_LIKE_ISO_GAUSS: return go_hmc<W, CW, SMCMC_LIKE_ISO_GAUSS>(p, s, sv);
        case SMCMC_LIKE_QUADFORM: return go_hmc<W, CW, SMCMC_LIKE_QUADFORM>(p, s, sv);
        case SMCMC_LIKE_ROSENBROCK: return go_hmc<W, CW, SMCMC_LIKE_ROSENBROCK>(p, s, sv);
        case SMCMC_LIKE_ASYM: return go_hmc_no_gradient<W, CW, SMCMC_LIKE_ASYM>(p, s, sv);
        case SMCMC_LIKE_HORRIFIC: return go_hmc_no_gradient<W, CW, SMCMC_LIKE_HORRIFIC>(p, s, sv);
        case SMCMC_LIKE_CONSTRAINED: return go_hmc_no_gradient<W, CW, SMCMC_LIKE_CONSTRAINED>(p, s, sv);
#if defined(SMCMC_USER_LIKELIHOOD_ANY_DIM) && defined(SMCMC_USER_GRADIENT)
        // a user likelihood with a gradient of its own (smcmc_user_gradient_at): types 0 / 1 / 4 in the plain instantiation
        case SMCMC_LIKE_USER: return go_hmc<W, CW, SMCMC_LIKE_USER>(p, s, sv);
#elif defined(SMCMC_USER_LIKELIHOOD_ANY_DIM)
        case SMCMC_LIKE_USER: return go_hmc_no_gradient<W, CW, SMCMC_LIKE_USER>(p, s, sv);
#endif
        default: return hipErrorInvalidValue;
    }
}

}  // namespace smcmc
