// smcmc_perchain_limits.h -- the dimensions SMCMC_MODE_PER_CHAIN serves, for the units that size or check its images
// without the kernels themselves (smcmc_perchain_inst.hip's staging and broadcast helpers).
#pragma once

namespace smcmc {

constexpr int kWgThreads = 512;              // one chain per workgroup (smcmc_perchain_wg.hip.h)
// Registers of covariance (and as many of decomposition) per thread in the largest class.  24 keeps every instantiation
// free of scratch: at 24 the kernel takes 246 of the 256 VGPRs a thread has at two wavefronts per SIMD, of which the
// chain's two matrices are 96.  The next classes do not fit: NE = 32 (D <= 180) spills 72 VGPRs, NE = 40 (D <= 201)
// spills 220 -- the matrices alone are 160 there, and the step's own working set is ~150.
constexpr int kWgMaxNE = 24;
constexpr int kWgMaxDim = 156;               // the largest D with D (D + 1) / 2 <= kWgThreads * kWgMaxNE
static_assert(kWgMaxDim * (kWgMaxDim + 1) / 2 <= kWgThreads * kWgMaxNE &&
              (kWgMaxDim + 1) * (kWgMaxDim + 2) / 2 > kWgThreads * kWgMaxNE, "kWgMaxDim");

}  // namespace smcmc
