// smcmc_event_sample_error.hpp -- the text behind smcmc_event_sample_last_error (include/smcmc.h), for the entry points of
// the event-sample family that live outside smcmc_event_sample.hip, which owns it (smcmc_event_predictive.hip).
#pragma once

#include <string>

namespace smcmc {

// what smcmc_event_sample_last_error gives this thread next; "" = the call was well formed
void es_set_last_error(const std::string& text);

}  // namespace smcmc
