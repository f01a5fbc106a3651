// smcmc_hmc_mfma_inst.hip -- the matrix-pipe HMC kernel (quadratic-form likelihood, fused order).
#include "smcmc_hmc_mfma_kernel.hip.h"

namespace smcmc {

namespace {
const HmcSaveArgs kNoSave = {nullptr, nullptr, 1, 0};
bool save_args_ok(const HmcParams& p, const HmcSaveArgs* sv) {
    return hmc_mfma_saves_in_kernel(p.dim) && sv->x != nullptr && sv->stride >= 1 && sv->first >= 0;
}
}  // namespace

hipError_t launch_hmc_mfma(const HmcParams& p, hipStream_t s, const HmcSaveArgs* sv) {
    const dim3 grid(p.npad / kMfCT), block(kMfW * kWave);
    if (sv != nullptr) {
        if (!save_args_ok(p, sv)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_mfma_kernel<1, true, true>), grid, block, 0, s, p, *sv);
    } else if (p.dim <= 128) hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_mfma_kernel<1>), grid, block, 0, s, p, kNoSave);
    else if (p.dim <= 256) hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_mfma_kernel<2>), grid, block, 0, s, p, kNoSave);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_mfma_kernel<4>), grid, block, 0, s, p, kNoSave);
    return hipGetLastError();
}

// the same layout in the reference's operation order (gradient on the vector pipe)
hipError_t launch_hmc_matrix_exact(const HmcParams& p, hipStream_t s, const HmcSaveArgs* sv) {
    const dim3 grid(p.npad / kMfCT), block(kMfW * kWave);
    if (sv != nullptr) {
        if (!save_args_ok(p, sv)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_mfma_kernel<1, false, true>), grid, block, 0, s, p, *sv);
    } else if (p.dim <= 128) hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_mfma_kernel<1, false>), grid, block, 0, s, p, kNoSave);
    else if (p.dim <= 256) hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_mfma_kernel<2, false>), grid, block, 0, s, p, kNoSave);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(hmc_mfma_kernel<4, false>), grid, block, 0, s, p, kNoSave);
    return hipGetLastError();
}

}  // namespace smcmc
