// smcmc_event_sample.hip -- smcmc_event_sample_evaluate and smcmc_event_template_evaluate (include/smcmc.h):
// SMCMC_LIKE_EVENT_SAMPLE and SMCMC_LIKE_EVENT_TEMPLATE evaluated on the host from the header the device kernels compile (include/smcmc_event_sample.h), for what the reference does outside
// Step(): Init()'s exposure ratio and WriteSimulation() (example/FakeLikelihood.H:107-143, 173-179).  No chain is
// stepped here.  Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

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

extern "C" const char* smcmc_event_sample_last_error(void) { return es_error.c_str(); }
