// smcmc_event_sample_host.hpp -- host side of SMCMC_LIKE_EVENT_SAMPLE and SMCMC_LIKE_EVENT_TEMPLATE: the rules of the caller's parameter array
// (smcmc.h), the engine's packed layout of it (include/smcmc_event_sample.h) and the likelihood evaluated on the host
// from that layout, the walk the device kernels make.
#pragma once

#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "smcmc.h"
#include "smcmc_event_sample.h"

namespace smcmc {

// nullptr when params[0 .. count) is a well-formed event sample, else what is wrong with it
inline const char* es_check(const double* p, size_t count) {
    if (!p || count < (size_t)SMCMC_ES_PARAM_HEADER)
        return "EVENT_SAMPLE needs {nevents, nbins, xmin, xmax, exposureRatio, separationCut, trueFakes, trueEfficiency, "
               "data[3][nbins], events[nevents][6]}";
    for (int i = 0; i < SMCMC_ES_PARAM_HEADER; ++i)
        if (!std::isfinite(p[i])) return "EVENT_SAMPLE: a header field is not finite";
    if (p[1] != std::floor(p[1]) || p[1] < 1.0 || p[1] > (double)SMCMC_EVENT_SAMPLE_MAX_BINS)
        return "EVENT_SAMPLE: nbins must be an integer from 1 to SMCMC_EVENT_SAMPLE_MAX_BINS";
    if (p[0] != std::floor(p[0]) || p[0] < 1.0 || p[0] > 1e8) return "EVENT_SAMPLE: nevents must be an integer, at least 1";
    const size_t nev = (size_t)p[0], nbins = (size_t)p[1];
    if (count != (size_t)SMCMC_ES_PARAM_HEADER + 3 * nbins + 6 * nev)
        return "EVENT_SAMPLE takes exactly 8 + 3 nbins + 6 nevents likelihood parameters";
    if (!(p[2] < p[3])) return "EVENT_SAMPLE: xmin must be below xmax";
    if (!(p[6] > 0.0 && p[6] < 1.0 && p[7] > 0.0 && p[7] < 1.0))
        return "EVENT_SAMPLE: trueFakes and trueEfficiency lie inside (0, 1)";
    for (size_t i = SMCMC_ES_PARAM_HEADER; i < count; ++i)
        if (!std::isfinite(p[i])) return "EVENT_SAMPLE: a field of the data or of an event is not finite";
    const double* ev = p + SMCMC_ES_PARAM_HEADER + 3 * nbins;
    for (size_t e = 0; e < nev; ++e) {
        const double* q = ev + 6 * e;
        if (!(q[0] > 0.0) || !(q[4] > 0.0) || !(q[5] > 0.0))
            return "EVENT_SAMPLE: Mass, TrueMass and TrueMassSigma of every event must be > 0";
        if (q[1] < 0.0) return "EVENT_SAMPLE: Type must be 0 (signal) or > 0 (background)";
    }
    return nullptr;
}

// ... when it is a well-formed sample of SMCMC_LIKE_EVENT_TEMPLATE: the same array and rules, and three more
inline const char* et_check(const double* p, size_t count) {
    if (const char* why = es_check(p, count)) return why;
    if (p[4] != 1.0) return "EVENT_TEMPLATE: exposureRatio must be exactly 1 (example2 has no exposure ratio)";
    const size_t nev = (size_t)p[0], nbins = (size_t)p[1];
    const double* ev = p + SMCMC_ES_PARAM_HEADER + 3 * nbins;
    size_t nsig = 0;
    for (size_t e = 0; e < nev; ++e) nsig += (ev[6 * e + 1] > 0.0) ? 0 : 1;
    if (nsig == 0) return "EVENT_TEMPLATE: at least one event must be signal (Type 0)";
    if (nsig == nev) return "EVENT_TEMPLATE: at least one event must be background (Type > 0)";
    return nullptr;
}

// the rules of `likelihood`'s parameter array (SMCMC_LIKE_EVENT_SAMPLE or SMCMC_LIKE_EVENT_TEMPLATE)
inline const char* es_check_like(int likelihood, const double* p, size_t count) {
    return likelihood == SMCMC_LIKE_EVENT_TEMPLATE ? et_check(p, count) : es_check(p, count);
}

// The packed layout of a checked parameter array.  by_class (SMCMC_LIKE_EVENT_TEMPLATE): the events stably partitioned,
// signal first, and their number in the header; no histogram of that likelihood takes events of both classes, so every
// sum keeps its order of additions.
inline void es_pack(const double* p, std::vector<double>& out, bool by_class = false) {
    const size_t nev = (size_t)p[0], nbins = (size_t)p[1];
    out.assign((size_t)SMCMC_ES_HEADER + 3 * nbins + (size_t)SMCMC_ES_EVENT * nev, 0.0);
    const double pi = 3.14159265358979323846;
    out[SMCMC_ES_H_NEVENTS] = p[0]; out[SMCMC_ES_H_NBINS] = p[1]; out[SMCMC_ES_H_XMIN] = p[2]; out[SMCMC_ES_H_XMAX] = p[3];
    out[SMCMC_ES_H_EXPOSURE] = p[4]; out[SMCMC_ES_H_CUT] = p[5]; out[SMCMC_ES_H_TRUE_FAKES] = p[6]; out[SMCMC_ES_H_TRUE_EFF] = p[7];
    out[SMCMC_ES_H_TAN_FAKES] = std::tan(pi * (p[6] - 0.5));        // SystematicCorrection.H:94
    out[SMCMC_ES_H_TAN_EFF] = std::tan(pi * (p[7] - 0.5));          // :106
    out[SMCMC_ES_H_RANGE] = p[3] - p[2];
    for (size_t i = 0; i < 3 * nbins; ++i) out[SMCMC_ES_HEADER + i] = p[SMCMC_ES_PARAM_HEADER + i];
    const double* ev = p + SMCMC_ES_PARAM_HEADER + 3 * nbins;
    double* dst = out.data() + SMCMC_ES_HEADER + 3 * nbins;
    size_t nsig = 0;
    if (by_class) {
        for (size_t e = 0; e < nev; ++e) nsig += (ev[6 * e + 1] > 0.0) ? 0 : 1;
        out[SMCMC_ES_H_NSIGNAL] = (double)nsig;
    }
    size_t at[2] = {0, nsig};                                       // the next packed slot of a signal / a background event
    for (size_t e = 0; e < nev; ++e) {
        const double* q = ev + 6 * e;
        const double mass = q[0], true_mass = q[4], true_sigma = q[5];
        const double nominalLogMass = smcmc_log(true_mass);                            // :57
        double nominalLogSigma = smcmc_log(true_mass + true_sigma);                    // :58
        nominalLogSigma = nominalLogSigma - nominalLogMass;                            // :59
        const double logMass = smcmc_log(mass);                                        // :61
        const double logSigma = (logMass - nominalLogMass) / nominalLogSigma;          // :62
        double* d = dst + (size_t)SMCMC_ES_EVENT * (by_class ? at[q[1] > 0.0 ? 1 : 0]++ : e);
        d[0] = nominalLogMass;
        d[1] = logMass - nominalLogMass;
        d[2] = logSigma;
        d[3] = q[2];
        d[4] = (double)((q[1] > 0.0 ? 2 : 0) + (q[3] > 0.0 ? 1 : 0));
        d[5] = 0.0;
    }
}

// log L at point[9] from the packed layout; hist (may be null): [3][nbins]
inline double es_evaluate_packed(const double* pk, const double* point, double* hist) {
    const int nev = (int)pk[SMCMC_ES_H_NEVENTS], nbins = (int)pk[SMCMC_ES_H_NBINS];
    smcmc_es_scalars s;
    smcmc_es_point_scalars(point, pk[SMCMC_ES_H_EXPOSURE], pk[SMCMC_ES_H_TRUE_FAKES], pk[SMCMC_ES_H_TRUE_EFF],
                           pk[SMCMC_ES_H_TAN_FAKES], pk[SMCMC_ES_H_TAN_EFF], &s);
    std::vector<double> h((size_t)3 * nbins, 0.0);
    const double* ev = pk + SMCMC_ES_HEADER + 3 * nbins;
    for (int e = 0; e < nev; ++e) {
        const double* q = ev + (size_t)SMCMC_ES_EVENT * e;
        const int cls = (int)q[4];
        const int b = smcmc_es_event_bin(q[0], q[1], q[2], q[3], cls >> 1, cls & 1, &s, nbins, pk[SMCMC_ES_H_XMIN],
                                         pk[SMCMC_ES_H_XMAX], pk[SMCMC_ES_H_RANGE], pk[SMCMC_ES_H_CUT]);
        if (b >= 0) h[b] = h[b] + s.weight[cls];
    }
    double logl = 0.0;
    for (int r = 0; r < 3 * nbins; ++r) logl += smcmc_es_bin_term(pk[SMCMC_ES_HEADER + r], h[r]);
    if (hist)
        for (int r = 0; r < 3 * nbins; ++r) hist[r] = h[r];
    return logl;
}

// SMCMC_LIKE_EVENT_TEMPLATE from the packed layout (made with by_class): log L at point[9]; hist (may be null): the
// expectation [3][nbins] before the clamp; parts (may be null): S[3][nbins], B[3][nbins], IS, IB, ws, wb.  The device
// kernels make this walk with these functions.
inline double et_evaluate_packed(const double* pk, const double* point, double* hist, double* parts) {
    const int nev = (int)pk[SMCMC_ES_H_NEVENTS], nbins = (int)pk[SMCMC_ES_H_NBINS], nsig = (int)pk[SMCMC_ES_H_NSIGNAL];
    const int rows = 3 * nbins;
    smcmc_es_scalars s;
    smcmc_et_point_scalars(point, pk[SMCMC_ES_H_TRUE_FAKES], pk[SMCMC_ES_H_TRUE_EFF], pk[SMCMC_ES_H_TAN_FAKES],
                           pk[SMCMC_ES_H_TAN_EFF], &s);
    std::vector<double> h((size_t)2 * rows, 0.0);                   // S, then B
    const double* ev = pk + SMCMC_ES_HEADER + rows;
    double integral[2], norm[2];
    for (int c = 0; c < 2; ++c) {
        double* hc = h.data() + (size_t)c * rows;
        for (int e = c ? nsig : 0; e < (c ? nev : nsig); ++e) {
            const double* q = ev + (size_t)SMCMC_ES_EVENT * e;
            const int cls = (int)q[4];
            const int b = smcmc_es_event_bin(q[0], q[1], q[2], q[3], cls >> 1, cls & 1, &s, nbins, pk[SMCMC_ES_H_XMIN],
                                             pk[SMCMC_ES_H_XMAX], pk[SMCMC_ES_H_RANGE], pk[SMCMC_ES_H_CUT]);
            if (b >= 0) hc[b] = hc[b] + s.weight[cls];
        }
        double sum[3];
        for (int k = 0; k < 3; ++k) {
            sum[k] = 0.0;
            for (int b = 0; b < nbins; ++b) sum[k] += hc[k * nbins + b];
        }
        integral[c] = smcmc_et_integral(sum[0], sum[1], sum[2]);
        norm[c] = smcmc_et_norm(point[c], integral[c]);
    }
    double logl = 0.0;
    for (int r = 0; r < rows; ++r) {
        const double mc = smcmc_et_mc(smcmc_et_mc_signal(norm[0], h[r]), norm[1], h[(size_t)rows + r]);
        if (hist) hist[r] = mc;
        logl += smcmc_es_bin_term(pk[SMCMC_ES_HEADER + r], mc);
    }
    if (parts) {
        for (int r = 0; r < 2 * rows; ++r) parts[r] = h[r];
        parts[2 * rows] = integral[0]; parts[2 * rows + 1] = integral[1];
        parts[2 * rows + 2] = norm[0]; parts[2 * rows + 3] = norm[1];
    }
    return smcmc_et_penalties(logl, point);
}

}  // namespace smcmc
