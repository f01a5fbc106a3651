// smcmc_selftest.hip -- device-side probes behind smcmc_selftest_* (include/smcmc.h).
//
// They exist so the parity tests can pin two hardware facts the engine relies on:
//   1. include/smcmc_detmath.h evaluates bit for bit the same on gfx950 as on the
//      host (IEEE + - * / sqrt fma, no contraction);
//   2. a chain of v_mfma_f64_16x16x4_f64 accumulates its K products in ascending k
//      with one fused multiply-add each -- the order the pooled moments are
//      defined in (oracle/ensemble_oracle.c).
#include <hip/hip_runtime.h>

#include <vector>

#include "smcmc.h"
#include "smcmc_detmath.h"
#include "smcmc_host.hpp"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ void detmath_kernel(int kind, int n, const double* __restrict__ x, const double* __restrict__ y,
                               double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = x[i];
    const double b = y ? y[i] : 0.0;
    double r = 0.0, s, c;
    switch (kind) {
        case 0: r = smcmc_log(a); break;
        case 1: r = smcmc_exp(a); break;
        case 2: smcmc_sincos2pi(a, &s, &c); r = s; break;
        case 3: smcmc_sincos2pi(a, &s, &c); r = c; break;
        case 4: r = smcmc_pow_small(a, b); break;
        case 5: r = __builtin_sqrt(a); break;
        case 6: r = a / b; break;
        case 7: smcmc_normal_pair((uint32_t)a, (uint32_t)b, &c, &s); r = c; break;   // words held as doubles
        case 8: smcmc_normal_pair((uint32_t)a, (uint32_t)b, &c, &s); r = s; break;
        case 9: r = smcmc_sqrt_mid(a); break;
        case 10: r = smcmc_erf(a); break;
        case 11: r = smcmc_atan(a); break;
        default: break;
    }
    out[i] = r;
}

// c[16][16] (row-major) = sum_k a[i][k] * b[k][j], a: [16][K], b: [K][16]; one wavefront.
__global__ void __launch_bounds__(64) mfma_chain_kernel(int K, const double* __restrict__ a,
                                                        const double* __restrict__ b, double* __restrict__ c) {
    const int lane = threadIdx.x;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const double av = a[(lane & 15) * K + k0 + (lane >> 4)];    // A[i = lane&15][k = lane>>4]
        const double bv = b[(k0 + (lane >> 4)) * 16 + (lane & 15)]; // B[k = lane>>4][j = lane&15]
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    // C/D: column = lane & 15, row = (lane >> 4) + 4*reg
#pragma unroll
    for (int r = 0; r < 4; ++r) c[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];
}

// c[4][16] = sum_k a[4][K] b[K][16] with v_mfma_f64_4x4x4_4b_f64: four 4x4 blocks per instruction,
// block blk = (lane >> 2) & 3 covering columns 4 blk .. 4 blk + 3, the same four rows for every block.
__global__ void __launch_bounds__(64) mfma_strip_kernel(int K, const double* __restrict__ a,
                                                        const double* __restrict__ b, double* __restrict__ c) {
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const double av = a[(lane & 3) * K + k0 + (lane >> 4)];     // A[i = lane&3][k = lane>>4], any block
        const double bv = b[(k0 + (lane >> 4)) * 16 + (lane & 15)]; // B[k = lane>>4][j = lane&15]
        acc = __builtin_amdgcn_mfma_f64_4x4x4f64(av, bv, acc, 0, 0, 0);
    }
    c[(lane >> 4) * 16 + (lane & 15)] = acc;                        // D[i = lane>>4][j = lane&15]
}

}  // namespace

using smcmc::DeviceBuffer;

extern "C" int smcmc_selftest_detmath(int device, int kind, int n, const double* x, const double* y, double* out) {
    if (n <= 0 || !x || !out || kind < 0 || kind > 11) return SMCMC_ERR_INVALID;
    if (device == -1) {
        // the host's evaluation of the same header (no device is touched)
        for (int i = 0; i < n; ++i) {
            switch (kind) {
                case 0: out[i] = smcmc_log(x[i]); break;
                case 1: out[i] = smcmc_exp(x[i]); break;
                case 10: out[i] = smcmc_erf(x[i]); break;
                case 11: out[i] = smcmc_atan(x[i]); break;
                default: return SMCMC_ERR_INVALID;
            }
        }
        return SMCMC_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return SMCMC_ERR_NO_DEVICE;
    smcmc::DeviceGuard guard(device);
    DeviceBuffer<double> dx, dy, dout;
    const size_t bytes = sizeof(double) * (size_t)n;
    if (dx.allocate(n) != hipSuccess || dout.allocate(n) != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice) != hipSuccess) return SMCMC_ERR_HIP;
    if (y && (dy.allocate(n) != hipSuccess || hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice) != hipSuccess)) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(detmath_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, kind, n, dx.get(), dy.get(), dout.get());
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) != hipSuccess) return SMCMC_ERR_HIP;
    return SMCMC_OK;
}

extern "C" int smcmc_selftest_mfma(int device, int K, const double* a, const double* b, double* c) {
    if (K <= 0 || (K & 3) || !a || !b || !c) return SMCMC_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return SMCMC_ERR_NO_DEVICE;
    smcmc::DeviceGuard guard(device);
    DeviceBuffer<double> da, db, dc;
    const size_t ab = 16 * (size_t)K;
    if (da.allocate(ab) != hipSuccess || db.allocate(ab) != hipSuccess || dc.allocate(256) != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpy(da, a, sizeof(double) * ab, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(db, b, sizeof(double) * ab, hipMemcpyHostToDevice) != hipSuccess)
        return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(mfma_chain_kernel, dim3(1), dim3(64), 0, nullptr, K, da.get(), db.get(), dc.get());
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpy(c, dc, sizeof(double) * 256, hipMemcpyDeviceToHost) != hipSuccess) return SMCMC_ERR_HIP;
    return SMCMC_OK;
}

extern "C" int smcmc_selftest_mfma_strip(int device, int K, const double* a, const double* b, double* c) {
    if (K <= 0 || (K & 3) || !a || !b || !c) return SMCMC_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return SMCMC_ERR_NO_DEVICE;
    smcmc::DeviceGuard guard(device);
    DeviceBuffer<double> da, db, dc;
    if (da.allocate(4 * (size_t)K) != hipSuccess || db.allocate(16 * (size_t)K) != hipSuccess || dc.allocate(64) != hipSuccess)
        return SMCMC_ERR_HIP;
    if (hipMemcpy(da, a, sizeof(double) * 4 * (size_t)K, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(db, b, sizeof(double) * 16 * (size_t)K, hipMemcpyHostToDevice) != hipSuccess)
        return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(mfma_strip_kernel, dim3(1), dim3(64), 0, nullptr, K, da.get(), db.get(), dc.get());
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpy(c, dc, sizeof(double) * 64, hipMemcpyDeviceToHost) != hipSuccess) return SMCMC_ERR_HIP;
    return SMCMC_OK;
}
