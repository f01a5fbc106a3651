// smcmc_event_sample_host.hpp -- host side of SMCMC_LIKE_EVENT_SAMPLE and SMCMC_LIKE_EVENT_TEMPLATE: the rules of the caller's parameter array
// (smcmc.h), the engine's packed layout of it (include/smcmc_event_sample.h) and the likelihood evaluated on the host
// from that layout, the walk the device kernels make.
#pragma once

#include <cmath>
#include <cstddef>
#include <string>
#include <utility>
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

// K^-1 of an n x n kernel matrix (row-major), as SMCMC_LIKE_EVENT_SHAPE defines it: TMatrixD::Invert restated as ROOT
// does it for a general matrix -- an LU decomposition with partial pivoting (rows), then the columns of the inverse by
// a forward and a back substitution each.  (The Gauss-Jordan elimination of smcmc_hmc_shared.hpp leaves K Kinv - I at
// 2.0e-6 for example3's signal kernel, cond_1 8.3e8, above n u cond_1 = 1.2e-6; this leaves 1e-8.)  Every operation is
// one IEEE operation in the order written.  false when a pivot is exactly zero or something that is not finite comes out.
inline bool esh_invert(const double* k, int n, std::vector<double>& out) {
    std::vector<double> a(k, k + (size_t)n * n);
    std::vector<int> perm((size_t)n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    for (int col = 0; col < n; ++col) {
        int piv = col;
        for (int r = col + 1; r < n; ++r)
            if (std::fabs(a[(size_t)r * n + col]) > std::fabs(a[(size_t)piv * n + col])) piv = r;
        if (a[(size_t)piv * n + col] == 0.0) return false;
        if (piv != col) {
            for (int c = 0; c < n; ++c) std::swap(a[(size_t)col * n + c], a[(size_t)piv * n + c]);
            std::swap(perm[col], perm[piv]);
        }
        const double d = a[(size_t)col * n + col];
        for (int r = col + 1; r < n; ++r) {
            const double f = a[(size_t)r * n + col] / d;
            a[(size_t)r * n + col] = f;                                 // L below the diagonal, U on and above it
            for (int c = col + 1; c < n; ++c) a[(size_t)r * n + c] -= f * a[(size_t)col * n + c];
        }
    }
    out.assign((size_t)n * n, 0.0);
    std::vector<double> x((size_t)n);
    for (int j = 0; j < n; ++j) {                                       // K x = e_j
        for (int i = 0; i < n; ++i) {                                   // L y = P e_j
            double s = (perm[i] == j) ? 1.0 : 0.0;
            for (int c = 0; c < i; ++c) s -= a[(size_t)i * n + c] * x[c];
            x[i] = s;
        }
        for (int i = n - 1; i >= 0; --i) {                              // U x = y
            double s = x[i];
            for (int c = i + 1; c < n; ++c) s -= a[(size_t)i * n + c] * x[c];
            x[i] = s / a[(size_t)i * n + i];
        }
        for (int i = 0; i < n; ++i) out[(size_t)i * n + j] = x[i];
    }
    for (double v : out)
        if (!std::isfinite(v)) return false;
    return true;
}

// ... when it is a well-formed sample of SMCMC_LIKE_EVENT_SHAPE (smcmc.h)
inline const char* esh_check(const double* p, size_t count) {
    const char* form = "EVENT_SHAPE needs {nevents, nbins, xmin, xmax, cutVeryClose, cutClose, trueFakes, trueEfficiency, bkgLow, "
                       "bkgHigh, sigLow, sigHigh, data[4][nbins], KB[11][11], KS[13][13], events[nevents][6]}";
    if (!p || count < (size_t)SMCMC_ESH_PARAM_HEADER) return form;
    for (int i = 0; i < SMCMC_ESH_PARAM_HEADER; ++i)
        if (!std::isfinite(p[i])) return "EVENT_SHAPE: a header field is not finite";
    if (p[1] != std::floor(p[1]) || p[1] < 1.0 || p[1] > (double)SMCMC_EVENT_SHAPE_MAX_BINS)
        return "EVENT_SHAPE: nbins must be an integer from 1 to SMCMC_EVENT_SHAPE_MAX_BINS";
    if (p[0] != std::floor(p[0]) || p[0] < 1.0 || p[0] > 1e8) return "EVENT_SHAPE: nevents must be an integer, at least 1";
    const size_t nev = (size_t)p[0], nbins = (size_t)p[1];
    if (count != (size_t)SMCMC_ESH_PARAM_HEADER + 4 * nbins + 121 + 169 + 6 * nev)
        return "EVENT_SHAPE takes exactly 12 + 4 nbins + 121 + 169 + 6 nevents likelihood parameters";
    if (!(p[2] < p[3])) return "EVENT_SHAPE: xmin must be below xmax";
    if (!(p[4] <= p[5])) return "EVENT_SHAPE: cutVeryClose must not be above cutClose";
    if (!(p[6] > 0.0 && p[6] < 1.0 && p[7] > 0.0 && p[7] < 1.0))
        return "EVENT_SHAPE: trueFakes and trueEfficiency lie inside (0, 1)";
    if (!(p[8] < p[9])) return "EVENT_SHAPE: bkgLow must be below bkgHigh";
    if (!(p[10] < p[11])) return "EVENT_SHAPE: sigLow must be below sigHigh";
    for (size_t i = SMCMC_ESH_PARAM_HEADER; i < count; ++i)
        if (!std::isfinite(p[i])) return "EVENT_SHAPE: a field of the data, of a kernel or of an event is not finite";
    const double* kb = p + SMCMC_ESH_PARAM_HEADER + 4 * nbins;
    const double* ks = kb + 121;
    for (int i = 0; i < SMCMC_ESH_NB; ++i)
        for (int j = 0; j < i; ++j)
            if (kb[i * SMCMC_ESH_NB + j] != kb[j * SMCMC_ESH_NB + i]) return "EVENT_SHAPE: the background's kernel is not symmetric";
    for (int i = 0; i < SMCMC_ESH_NS; ++i)
        for (int j = 0; j < i; ++j)
            if (ks[i * SMCMC_ESH_NS + j] != ks[j * SMCMC_ESH_NS + i]) return "EVENT_SHAPE: the signal's kernel is not symmetric";
    const double* ev = ks + 169;
    size_t nsig = 0;
    for (size_t e = 0; e < nev; ++e) {
        const double* q = ev + 6 * e;
        if (!(q[0] > 0.0) || !(q[4] > 0.0) || !(q[5] > 0.0))
            return "EVENT_SHAPE: Mass, TrueMass and TrueMassSigma of every event must be > 0";
        if (q[1] < 0.0) return "EVENT_SHAPE: Type must be 0 (signal) or > 0 (background)";
        nsig += (q[1] > 0.0) ? 0 : 1;
    }
    if (nsig == 0) return "EVENT_SHAPE: at least one event must be signal (Type 0)";
    if (nsig == nev) return "EVENT_SHAPE: at least one event must be background (Type > 0)";
    std::vector<double> inv;
    if (!esh_invert(kb, SMCMC_ESH_NB, inv)) return "EVENT_SHAPE: the background's kernel cannot be inverted";
    if (!esh_invert(ks, SMCMC_ESH_NS, inv)) return "EVENT_SHAPE: the signal's kernel cannot be inverted";
    return nullptr;
}

// the rules of `likelihood`'s parameter array (SMCMC_LIKE_EVENT_SAMPLE, _TEMPLATE or _SHAPE)
inline const char* es_check_like(int likelihood, const double* p, size_t count) {
    if (likelihood == SMCMC_LIKE_EVENT_SHAPE) return esh_check(p, count);
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

// The packed layout of a checked SMCMC_LIKE_EVENT_SHAPE array (include/smcmc_event_shape.h): the events partitioned by
// class, the two kernels inverted, every event located on its class's shape.
inline void esh_pack(const double* p, std::vector<double>& out) {
    const size_t nev = (size_t)p[0], nbins = (size_t)p[1];
    out.assign((size_t)SMCMC_ESH_EVENTS(nbins) + (size_t)SMCMC_ESH_EVENT * nev, 0.0);
    const double pi = 3.14159265358979323846;
    out[SMCMC_ES_H_NEVENTS] = p[0]; out[SMCMC_ES_H_NBINS] = p[1]; out[SMCMC_ES_H_XMIN] = p[2]; out[SMCMC_ES_H_XMAX] = p[3];
    out[SMCMC_ES_H_EXPOSURE] = 1.0; out[SMCMC_ES_H_CUT] = p[5]; out[SMCMC_ESH_H_CUT_VERY_CLOSE] = p[4];
    out[SMCMC_ES_H_TRUE_FAKES] = p[6]; out[SMCMC_ES_H_TRUE_EFF] = p[7];
    out[SMCMC_ES_H_TAN_FAKES] = std::tan(pi * (p[6] - 0.5));        // example3/SystematicCorrection.H:94
    out[SMCMC_ES_H_TAN_EFF] = std::tan(pi * (p[7] - 0.5));          // :110
    out[SMCMC_ES_H_RANGE] = p[3] - p[2];
    for (size_t i = 0; i < 4 * nbins; ++i) out[SMCMC_ES_HEADER + i] = p[SMCMC_ESH_PARAM_HEADER + i];
    const double* kb = p + SMCMC_ESH_PARAM_HEADER + 4 * nbins;
    const double* ks = kb + 121;
    std::vector<double> inv;
    esh_invert(kb, SMCMC_ESH_NB, inv);
    for (size_t i = 0; i < 121; ++i) out[SMCMC_ESH_KINV_B(nbins) + i] = inv[i];
    esh_invert(ks, SMCMC_ESH_NS, inv);
    for (size_t i = 0; i < 169; ++i) out[SMCMC_ESH_KINV_S(nbins) + i] = inv[i];
    double* cb = out.data() + SMCMC_ESH_CENTRE_B(nbins);
    double* cs = out.data() + SMCMC_ESH_CENTRE_S(nbins);
    for (int i = 0; i < SMCMC_ESH_NB; ++i) cb[i] = smcmc_esh_centre(p[8], p[9], SMCMC_ESH_NB, i);
    for (int i = 0; i < SMCMC_ESH_NS; ++i) cs[i] = smcmc_esh_centre(p[10], p[11], SMCMC_ESH_NS, i);
    const double* ev = ks + 169;
    double* dst = out.data() + SMCMC_ESH_EVENTS(nbins);
    size_t nsig = 0;
    for (size_t e = 0; e < nev; ++e) nsig += (ev[6 * e + 1] > 0.0) ? 0 : 1;
    out[SMCMC_ES_H_NSIGNAL] = (double)nsig;
    size_t at[2] = {0, nsig};                                       // the next packed slot of a signal / a background event
    for (size_t e = 0; e < nev; ++e) {
        const double* q = ev + 6 * e;
        const double mass = q[0], true_mass = q[4], true_sigma = q[5];
        const double nominalLogMass = smcmc_log(true_mass);                            // :54
        double nominalLogSigma = smcmc_log(true_mass + true_sigma);                    // :55
        nominalLogSigma = nominalLogSigma - nominalLogMass;                            // :56
        const double logMass = smcmc_log(mass);                                        // :58
        const double logSigma = (logMass - nominalLogMass) / nominalLogSigma;          // :59
        const int bkg = q[1] > 0.0 ? 1 : 0;
        double* d = dst + (size_t)SMCMC_ESH_EVENT * at[bkg]++;
        d[0] = nominalLogMass;
        d[1] = logMass - nominalLogMass;
        d[2] = logSigma;
        d[3] = q[2];
        d[4] = (double)(2 * bkg + (q[3] > 0.0 ? 1 : 0));
        int k, clamped;
        double dx;
        if (bkg) smcmc_esh_locate(mass, p[8], p[9], SMCMC_ESH_NB, cb, &k, &dx, &clamped);     // :104, 120: the uncorrected mass
        else smcmc_esh_locate(mass, p[10], p[11], SMCMC_ESH_NS, cs, &k, &dx, &clamped);
        d[5] = (double)k;
        d[6] = dx;
        d[7] = (double)clamped;
    }
}

// SMCMC_LIKE_EVENT_SHAPE from the packed layout: log L at point[31]; hist (may be null): the expectation [4][nbins]
// before the clamp; parts (may be null): S[4][nbins], B[4][nbins], IS, IB, ws, wb, penalty(B), penalty(S), KinvB, KinvS.
// The device kernels make this walk with these functions.
inline double esh_evaluate_packed(const double* pk, const double* point, double* hist, double* parts) {
    const int nev = (int)pk[SMCMC_ES_H_NEVENTS], nbins = (int)pk[SMCMC_ES_H_NBINS], nsig = (int)pk[SMCMC_ES_H_NSIGNAL];
    const int rows = 4 * nbins;
    smcmc_es_scalars s;
    smcmc_esh_point_scalars(point, pk[SMCMC_ES_H_TRUE_FAKES], pk[SMCMC_ES_H_TRUE_EFF], pk[SMCMC_ES_H_TAN_FAKES],
                            pk[SMCMC_ES_H_TAN_EFF], &s);
    double yb[SMCMC_ESH_NB], ys[SMCMC_ESH_NS], slb[SMCMC_ESH_NB], sls[SMCMC_ESH_NS];
    const double* cb = pk + SMCMC_ESH_CENTRE_B(nbins);
    const double* cs = pk + SMCMC_ESH_CENTRE_S(nbins);
    for (int i = 0; i < SMCMC_ESH_NB; ++i) yb[i] = smcmc_esh_control_b(point, i);
    for (int i = 0; i < SMCMC_ESH_NS; ++i) ys[i] = smcmc_esh_control_s(point, i);
    for (int i = 0; i + 1 < SMCMC_ESH_NB; ++i) slb[i] = smcmc_esh_slope(yb[i], yb[i + 1], cb[i], cb[i + 1]);
    for (int i = 0; i + 1 < SMCMC_ESH_NS; ++i) sls[i] = smcmc_esh_slope(ys[i], ys[i + 1], cs[i], cs[i + 1]);
    slb[SMCMC_ESH_NB - 1] = sls[SMCMC_ESH_NS - 1] = 0.0;           // (a clamped event's: never read into a value)
    std::vector<double> h((size_t)2 * rows, 0.0);                   // S, then B
    const double* ev = pk + SMCMC_ESH_EVENTS(nbins);
    double integral[2], norm[2];
    for (int c = 0; c < 2; ++c) {
        double* hc = h.data() + (size_t)c * rows;
        const double* y = c ? yb : ys;
        const double* sl = c ? slb : sls;
        for (int e = c ? nsig : 0; e < (c ? nev : nsig); ++e) {
            const double* q = ev + (size_t)SMCMC_ESH_EVENT * e;
            const int cls = (int)q[4], k = (int)q[5];
            const int b = smcmc_esh_event_bin(q[0], q[1], q[2], q[3], cls >> 1, cls & 1, &s, nbins, pk[SMCMC_ES_H_XMIN],
                                              pk[SMCMC_ES_H_XMAX], pk[SMCMC_ES_H_RANGE], pk[SMCMC_ESH_H_CUT_VERY_CLOSE],
                                              pk[SMCMC_ES_H_CUT]);
            const double w = smcmc_esh_weight(s.weight[cls], smcmc_esh_shape(y[k], sl[k], q[6], q[7] != 0.0));
            if (b >= 0) hc[b] = hc[b] + w;
        }
        double sum[4];
        for (int k = 0; k < 4; ++k) {
            sum[k] = 0.0;
            for (int b = 0; b < nbins; ++b) sum[k] += hc[k * nbins + b];
        }
        integral[c] = smcmc_esh_integral(sum[0], sum[1], sum[2], sum[3]);
        norm[c] = smcmc_et_norm(point[c], integral[c]);
    }
    double logl = 0.0;
    for (int r = 0; r < rows; ++r) {
        const double mc = smcmc_et_mc(smcmc_et_mc_signal(norm[0], h[r]), norm[1], h[(size_t)rows + r]);
        if (hist) hist[r] = mc;
        logl += smcmc_es_bin_term(pk[SMCMC_ES_HEADER + r], mc);
    }
    const double pen_b = smcmc_esh_gp_penalty(yb, pk + SMCMC_ESH_KINV_B(nbins), SMCMC_ESH_NB);
    const double pen_s = smcmc_esh_gp_penalty(ys, pk + SMCMC_ESH_KINV_S(nbins), SMCMC_ESH_NS);
    if (parts) {
        for (int r = 0; r < 2 * rows; ++r) parts[r] = h[r];
        double* t = parts + 2 * rows;
        t[0] = integral[0]; t[1] = integral[1]; t[2] = norm[0]; t[3] = norm[1]; t[4] = pen_b; t[5] = pen_s;
        for (int i = 0; i < 121 + 169; ++i) t[6 + i] = pk[SMCMC_ESH_KINV_B(nbins) + i];
    }
    return smcmc_esh_penalties(logl, point, pen_b, pen_s);
}

}  // namespace smcmc
