// smcmc_host.hpp -- host plumbing shared by the engines (smcmc_engine.hip, smcmc_hmc_engine.hip, smcmc_vaat_engine.hip)
// and the standalone entry points: owning device buffers, the device guard, error reporting, the choice of the
// register-resident kernel family, a fill kernel and the format rules of the built-in likelihoods' parameters.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <string>
#include <vector>

#include "smcmc.h"
#include "smcmc_event_sample_host.hpp"
#include "smcmc_kernels.hip.h"   // SMCMC_FOR_EACH_DP

namespace smcmc {

// One owning, move-only allocation: device memory (hipMalloc / hipFree) or, with Pinned, page-locked host memory
// (hipHostMalloc / hipHostFree).  Reads as a T* wherever a raw pointer is expected (kernel parameters, copies).
template <typename T, bool Pinned = false>
class Buffer {
public:
    Buffer() = default;
    ~Buffer() { release(); }
    Buffer(Buffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;

    // n elements, uninitialised; what the buffer held before is freed first.  Empty on failure.
    hipError_t allocate(size_t n) {
        release();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        n_ = n;
        return hipSuccess;
    }
    size_t size() const { return n_; }
    T* get() const { return p_; }
    operator T*() const { return p_; }

private:
    void release() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

// Every entry point that touches the device runs on the engine's own device and leaves the
// caller's current device as it found it (two engines on two devices may share a thread).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = (hipSetDevice(device) == hipSuccess);
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ON_DEVICE(h) ::smcmc::DeviceGuard device_guard_((h)->device)

// the engine's last error (smcmc_*_last_error), and the status the entry point returns
template <typename H>
int fail(H* h, int status, const std::string& msg) {
    if (h) h->error = msg;
    return status;
}

#define HIP_TRY(h, expr)                                                                                  \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return ::smcmc::fail((h), SMCMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// register-resident kernel families, smallest first (SMCMC_FOR_EACH_DP)
#define SMCMC_DP_ENTRY(n) n,
constexpr int kDPList[] = {SMCMC_FOR_EACH_DP(SMCMC_DP_ENTRY)};
#undef SMCMC_DP_ENTRY
constexpr int kNumDP = sizeof(kDPList) / sizeof(kDPList[0]);

// the likelihoods over a simulated event sample (smcmc_event_sample.h): one parameter array, one packed layout
inline bool event_likelihood(int like) {
    return like == SMCMC_LIKE_EVENT_SAMPLE || like == SMCMC_LIKE_EVENT_TEMPLATE || like == SMCMC_LIKE_EVENT_SHAPE;
}
// the one dimension an event likelihood has: the nine systematic parameters, or example3's 31
inline int event_likelihood_dim(int like) { return like == SMCMC_LIKE_EVENT_SHAPE ? SMCMC_ESH_DIM : SMCMC_ES_DIM; }

inline bool stress_likelihood(int like) {
    return like == SMCMC_LIKE_ASYM || like == SMCMC_LIKE_HORRIFIC || like == SMCMC_LIKE_CONSTRAINED;
}

// the register-array size of the kernel family serving `dim`, or -1 above the largest (the large-dimension kernels)
inline int pick_dp(int dim, int like) {
    // the stress likelihoods are instantiated for the 31- and 63-wide families only (launch_step)
    for (int i = 0; i < kNumDP; ++i)
        if (dim <= kDPList[i] && (!stress_likelihood(like) || kDPList[i] == 31 || kDPList[i] == 63)) return kDPList[i];
    return -1;
}

// A kernel whose workgroup takes more dynamic LDS than the default limit (the headline step kernels: StepWorkgroupLds of
// smcmc_step_deal.h) has the limit raised before its first launch.  The attribute belongs to the function on one device,
// so it is set once per call site (`Site`: one tag type per kernel, which the launcher's template gives for nothing) and
// device; a second thread that gets there at the same time sets it again, to the same value.
template <typename Site>
hipError_t raise_dynamic_lds_once(const void* kernel, int bytes) {
    constexpr int kMaxDevices = 64;
    static std::atomic<bool> done[kMaxDevices];
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    const bool tracked = device >= 0 && device < kMaxDevices;
    if (tracked && done[device].load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && tracked) done[device].store(true, std::memory_order_release);
    return e;
}

template <typename T>
__global__ void fill_kernel(T* dst, size_t n, T v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = v;
}

// dst[0 .. n) = v on the stream
template <typename T>
hipError_t fill(T* dst, size_t n, T v, hipStream_t stream) {
    const int threads = 256;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fill_kernel<T>), dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0,
                       stream, dst, n, v);
    return hipGetLastError();
}

// The format of the built-in likelihoods' parameters (h->like_params for h->dim dimensions), the same in every engine.
// On success `prm` holds what the device reads for ROSENBROCK, ASYM and CONSTRAINED, defaults filled in, and a user
// likelihood's parameters as given; it stays empty for the others.  QUADFORM's Error matrix and EVENT_SAMPLE's sample
// are only checked: every engine packs the matrix in its own layout, the Metropolis engine the sample.  user_max / user_rule: the engine's own limit for SMCMC_LIKE_USER and its message.
template <typename H>
int check_like_params(H* h, int like, size_t user_max, const char* user_rule, std::vector<double>& prm) {
    const std::vector<double>& p = h->like_params;
    prm.clear();
    switch (like) {
        case SMCMC_LIKE_QUADFORM:
            if (p.size() != (size_t)h->dim * h->dim)
                return fail(h, SMCMC_ERR_INVALID, "QUADFORM needs dim*dim likelihood parameters (the Error matrix)");
            break;
        case SMCMC_LIKE_ROSENBROCK:
            prm = {p.empty() ? 100.0 : p[0]};                      // ROSEN_B, THardLogLikelihood.H:53
            break;
        case SMCMC_LIKE_ASYM:
            if (p.empty()) prm = {-1.0, 100.0};                    // TAsymLogLikelihood.H:17-18
            else if (p.size() == 2) prm = p;
            else return fail(h, SMCMC_ERR_INVALID, "ASYM takes {positiveSlope, negativeSlope}");
            break;
        case SMCMC_LIKE_CONSTRAINED:
            if (p.size() != 2 + 2 * (size_t)h->dim)
                return fail(h, SMCMC_ERR_INVALID,
                            "CONSTRAINED needs {SummedValues, SummedConstraint, ExpectedValues[dim], PriorConstraints[dim]}");
            prm = p;
            break;
        case SMCMC_LIKE_EVENT_SAMPLE:
        case SMCMC_LIKE_EVENT_TEMPLATE:
        case SMCMC_LIKE_EVENT_SHAPE: {
            // only checked, like QUADFORM's matrix: the engine packs the sample in a layout of its own (es_pack)
            const char* why = es_check_like(like, p.data(), p.size());
            if (why) return fail(h, SMCMC_ERR_INVALID, why);
            break;
        }
        case SMCMC_LIKE_USER:
            if (p.size() > user_max) return fail(h, SMCMC_ERR_INVALID, user_rule);
            prm = p;
            break;
        default: break;
    }
    return SMCMC_OK;
}

}  // namespace smcmc
