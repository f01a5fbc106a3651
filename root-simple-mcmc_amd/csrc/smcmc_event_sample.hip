// smcmc_event_sample.hip -- smcmc_event_sample_evaluate, smcmc_event_template_evaluate and smcmc_event_shape_evaluate
// (include/smcmc.h): the three likelihoods over a simulated event sample evaluated on the host from the header the device
// kernels compile (include/smcmc_event_sample.h), for what the reference does outside
// Step(): Init()'s exposure ratio and WriteSimulation() (example/FakeLikelihood.H:107-143, 173-179).  No chain is
// stepped here.  Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "smcmc.h"
#include "smcmc_event_sample_error.hpp"
#include "smcmc_event_sample_host.hpp"

namespace {
thread_local std::string es_error;

// what the three evaluators do before they walk: the arguments, the rules of the array, the packed layout
int es_prepare(const char* entry, int likelihood, const double* params, int count, const double* point, const double* logl,
               std::vector<double>& packed) {
    if (!point || !logl || count < 0) {
        es_error = std::string(entry) + ": point and logl must be given";
        return SMCMC_ERR_INVALID;
    }
    const char* why = smcmc::es_check_like(likelihood, params, (size_t)count);
    if (why) {
        es_error = why;
        return SMCMC_ERR_INVALID;
    }
    smcmc::es_pack(likelihood, params, packed);
    es_error.clear();
    return SMCMC_OK;
}
}

void smcmc::es_set_last_error(const std::string& text) { es_error = text; }

extern "C" int smcmc_event_sample_evaluate(const double* params, int count, const double* point, double* logl, double* hist) {
    std::vector<double> packed;
    const int st = es_prepare("smcmc_event_sample_evaluate", SMCMC_LIKE_EVENT_SAMPLE, params, count, point, logl, packed);
    if (st == SMCMC_OK) *logl = smcmc::es_evaluate_packed(packed.data(), point, hist);
    return st;
}

extern "C" int smcmc_event_template_evaluate(const double* params, int count, const double* point, double* logl, double* hist,
                                             double* parts) {
    std::vector<double> packed;
    const int st = es_prepare("smcmc_event_template_evaluate", SMCMC_LIKE_EVENT_TEMPLATE, params, count, point, logl, packed);
    if (st == SMCMC_OK) *logl = smcmc::es_two_pass_packed(false, packed.data(), point, hist, parts);
    return st;
}

extern "C" int smcmc_event_shape_evaluate(const double* params, int count, const double* point, double* logl, double* hist,
                                          double* parts) {
    std::vector<double> packed;
    const int st = es_prepare("smcmc_event_shape_evaluate", SMCMC_LIKE_EVENT_SHAPE, params, count, point, logl, packed);
    if (st == SMCMC_OK) *logl = smcmc::es_two_pass_packed(true, packed.data(), point, hist, parts);
    return st;
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
