// smcmc_event_sample.hip -- smcmc_event_sample_evaluate and smcmc_event_template_evaluate (include/smcmc.h):
// SMCMC_LIKE_EVENT_SAMPLE and SMCMC_LIKE_EVENT_TEMPLATE evaluated on the host from the header the device kernels compile (include/smcmc_event_sample.h), for what the reference does outside
// Step(): Init()'s exposure ratio and WriteSimulation() (example/FakeLikelihood.H:107-143, 173-179).  No chain is
// stepped here.  Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "smcmc.h"
#include "smcmc_event_sample_host.hpp"

namespace {
thread_local std::string es_error;
}

extern "C" int smcmc_event_sample_evaluate(const double* params, int count, const double* point, double* logl, double* hist) {
    if (!point || !logl || count < 0) {
        es_error = "smcmc_event_sample_evaluate: point and logl must be given";
        return SMCMC_ERR_INVALID;
    }
    const char* why = smcmc::es_check(params, (size_t)count);
    if (why) {
        es_error = why;
        return SMCMC_ERR_INVALID;
    }
    std::vector<double> packed;
    smcmc::es_pack(params, packed);
    *logl = smcmc::es_evaluate_packed(packed.data(), point, hist);
    es_error.clear();
    return SMCMC_OK;
}

extern "C" int smcmc_event_template_evaluate(const double* params, int count, const double* point, double* logl, double* hist,
                                             double* parts) {
    if (!point || !logl || count < 0) {
        es_error = "smcmc_event_template_evaluate: point and logl must be given";
        return SMCMC_ERR_INVALID;
    }
    const char* why = smcmc::et_check(params, (size_t)count);
    if (why) {
        es_error = why;
        return SMCMC_ERR_INVALID;
    }
    std::vector<double> packed;
    smcmc::es_pack(params, packed, true);
    *logl = smcmc::et_evaluate_packed(packed.data(), point, hist, parts);
    es_error.clear();
    return SMCMC_OK;
}

extern "C" int smcmc_event_shape_evaluate(const double* params, int count, const double* point, double* logl, double* hist,
                                          double* parts) {
    if (!point || !logl || count < 0) {
        es_error = "smcmc_event_shape_evaluate: point and logl must be given";
        return SMCMC_ERR_INVALID;
    }
    const char* why = smcmc::esh_check(params, (size_t)count);
    if (why) {
        es_error = why;
        return SMCMC_ERR_INVALID;
    }
    std::vector<double> packed;
    smcmc::esh_pack(params, packed);
    *logl = smcmc::esh_evaluate_packed(packed.data(), point, hist, parts);
    es_error.clear();
    return SMCMC_OK;
}

extern "C" int smcmc_event_shape_gp_value(double low, double high, int n, const double* y, double x, double* value) {
    if (!y || !value || n < 1 || !(low < high) || !std::isfinite(low) || !std::isfinite(high)) {
        es_error = "smcmc_event_shape_gp_value: n >= 1 control values over low < high";
        return SMCMC_ERR_INVALID;
    }
    std::vector<double> c((size_t)n);
    for (int i = 0; i < n; ++i) c[i] = smcmc_esh_centre(low, high, n, i);
    int k, clamped;
    double dx;
    smcmc_esh_locate(x, low, high, n, c.data(), &k, &dx, &clamped);
    const double slope = clamped ? 0.0 : smcmc_esh_slope(y[k], y[k + 1], c[k], c[k + 1]);
    *value = smcmc_esh_shape(y[k], slope, dx, clamped);
    es_error.clear();
    return SMCMC_OK;
}

extern "C" int smcmc_event_shape_gp_penalty(const double* kernel, int n, const double* y, double* penalty, double* inverse) {
    if (!kernel || !y || !penalty || n < 1 || n > 64) {
        es_error = "smcmc_event_shape_gp_penalty: an n x n kernel and n control values, n from 1 to 64";
        return SMCMC_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j)
            if (!std::isfinite(kernel[i * n + j]) || kernel[i * n + j] != kernel[j * n + i]) {
                es_error = "smcmc_event_shape_gp_penalty: the kernel must be finite and exactly symmetric";
                return SMCMC_ERR_INVALID;
            }
    std::vector<double> inv;
    if (!smcmc::esh_invert(kernel, n, inv)) {
        es_error = "smcmc_event_shape_gp_penalty: the kernel cannot be inverted";
        return SMCMC_ERR_INVALID;
    }
    *penalty = smcmc_esh_gp_penalty(y, inv.data(), n);
    if (inverse)
        for (size_t i = 0; i < inv.size(); ++i) inverse[i] = inv[i];
    es_error.clear();
    return SMCMC_OK;
}

extern "C" const char* smcmc_event_sample_last_error(void) { return es_error.c_str(); }
