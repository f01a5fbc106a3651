// smcmc_event_sample_host.hpp -- host side of the likelihoods over a simulated event sample, SMCMC_LIKE_EVENT_SAMPLE,
// _TEMPLATE and _SHAPE: the rules of the caller's parameter array (smcmc.h), the engine's packed layout of it
// (include/smcmc_event_sample.h, smcmc_event_shape.h) and the likelihood evaluated on the host from that layout, the walk
// the device kernels make.
#pragma once

#include <cmath>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "smcmc.h"
#include "smcmc_event_sample.h"

namespace smcmc {

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

// What tells the three parameter arrays apart.  `name` is what the common rules call the array in their messages: the
// template's array is the event sample's, and so are their words for it.
struct EventForm {
    const char* name;
    int header, nh, kernels;        // doubles in front of the data; histograms; doubles between the data and the events
    const char* count;              // the exact count, as the message states it
    const char* fields;             // what lies behind the header
    bool two_pass;                  // SMCMC_LIKE_EVENT_TEMPLATE and _SHAPE: the events by class, one of each at least
};
inline EventForm event_form(int likelihood) {
    if (likelihood == SMCMC_LIKE_EVENT_SHAPE)
        return {"EVENT_SHAPE", SMCMC_ESH_PARAM_HEADER, 4, 121 + 169, "12 + 4 nbins + 121 + 169 + 6 nevents",
                "the data, of a kernel or of an event", true};
    return {"EVENT_SAMPLE", SMCMC_ES_PARAM_HEADER, 3, 0, "8 + 3 nbins + 6 nevents", "the data or of an event",
            likelihood == SMCMC_LIKE_EVENT_TEMPLATE};
}

// The rules of `likelihood`'s parameter array (SMCMC_LIKE_EVENT_SAMPLE, _TEMPLATE or _SHAPE; smcmc.h states them):
// nullptr when params[0 .. count) is well formed, else what is wrong with it (the text lives until the thread's next call).
inline const char* es_check_like(int likelihood, const double* p, size_t count) {
    static thread_local std::string why;
    const bool shape = likelihood == SMCMC_LIKE_EVENT_SHAPE, tmpl = likelihood == SMCMC_LIKE_EVENT_TEMPLATE;
    const EventForm f = event_form(likelihood);
    const std::string name = f.name;
    const auto fail = [&](const std::string& text) { why = text; return why.c_str(); };
    if (!p || count < (size_t)f.header)
        return shape ? "EVENT_SHAPE needs {nevents, nbins, xmin, xmax, cutVeryClose, cutClose, trueFakes, trueEfficiency, bkgLow, "
                       "bkgHigh, sigLow, sigHigh, data[4][nbins], KB[11][11], KS[13][13], events[nevents][6]}"
                     : "EVENT_SAMPLE needs {nevents, nbins, xmin, xmax, exposureRatio, separationCut, trueFakes, trueEfficiency, "
                       "data[3][nbins], events[nevents][6]}";
    for (int i = 0; i < f.header; ++i)
        if (!std::isfinite(p[i])) return fail(name + ": a header field is not finite");
    const int max_bins = shape ? SMCMC_EVENT_SHAPE_MAX_BINS : SMCMC_EVENT_SAMPLE_MAX_BINS;
    if (p[1] != std::floor(p[1]) || p[1] < 1.0 || p[1] > (double)max_bins)
        return fail(name + ": nbins must be an integer from 1 to SMCMC_" + name + "_MAX_BINS");
    if (p[0] != std::floor(p[0]) || p[0] < 1.0 || p[0] > 1e8) return fail(name + ": nevents must be an integer, at least 1");
    const size_t nev = (size_t)p[0], nbins = (size_t)p[1];
    if (count != (size_t)f.header + f.nh * nbins + f.kernels + 6 * nev)
        return fail(name + " takes exactly " + f.count + " likelihood parameters");
    if (!(p[2] < p[3])) return fail(name + ": xmin must be below xmax");
    if (shape && !(p[4] <= p[5])) return "EVENT_SHAPE: cutVeryClose must not be above cutClose";
    if (!(p[6] > 0.0 && p[6] < 1.0 && p[7] > 0.0 && p[7] < 1.0))
        return fail(name + ": trueFakes and trueEfficiency lie inside (0, 1)");
    if (shape && !(p[8] < p[9])) return "EVENT_SHAPE: bkgLow must be below bkgHigh";
    if (shape && !(p[10] < p[11])) return "EVENT_SHAPE: sigLow must be below sigHigh";
    for (size_t i = f.header; i < count; ++i)
        if (!std::isfinite(p[i])) return fail(name + ": a field of " + f.fields + " is not finite");
    const double* kb = p + f.header + f.nh * nbins;                 // (EVENT_SHAPE's two kernels)
    const double* ks = kb + 121;
    if (shape) {
        for (int i = 0; i < SMCMC_ESH_NB; ++i)
            for (int j = 0; j < i; ++j)
                if (kb[i * SMCMC_ESH_NB + j] != kb[j * SMCMC_ESH_NB + i]) return "EVENT_SHAPE: the background's kernel is not symmetric";
        for (int i = 0; i < SMCMC_ESH_NS; ++i)
            for (int j = 0; j < i; ++j)
                if (ks[i * SMCMC_ESH_NS + j] != ks[j * SMCMC_ESH_NS + i]) return "EVENT_SHAPE: the signal's kernel is not symmetric";
    }
    const double* ev = kb + f.kernels;
    size_t nsig = 0;
    for (size_t e = 0; e < nev; ++e) {
        const double* q = ev + 6 * e;
        if (!(q[0] > 0.0) || !(q[4] > 0.0) || !(q[5] > 0.0))
            return fail(name + ": Mass, TrueMass and TrueMassSigma of every event must be > 0");
        if (q[1] < 0.0) return fail(name + ": Type must be 0 (signal) or > 0 (background)");
        nsig += (q[1] > 0.0) ? 0 : 1;
    }
    if (tmpl && p[4] != 1.0) return "EVENT_TEMPLATE: exposureRatio must be exactly 1 (example2 has no exposure ratio)";
    if (f.two_pass) {
        const std::string own = shape ? "EVENT_SHAPE" : "EVENT_TEMPLATE";
        if (nsig == 0) return fail(own + ": at least one event must be signal (Type 0)");
        if (nsig == nev) return fail(own + ": at least one event must be background (Type > 0)");
    }
    if (shape) {
        std::vector<double> inv;
        if (!esh_invert(kb, SMCMC_ESH_NB, inv)) return "EVENT_SHAPE: the background's kernel cannot be inverted";
        if (!esh_invert(ks, SMCMC_ESH_NS, inv)) return "EVENT_SHAPE: the signal's kernel cannot be inverted";
    }
    return nullptr;
}

// The packed layout of a checked parameter array of `likelihood` (include/smcmc_event_sample.h, smcmc_event_shape.h).
// The two-pass likelihoods' events are stably partitioned by class, signal first, and the signal's number goes to the
// header: no histogram of theirs takes events of both classes, so every sum keeps its order of additions.  The shape's
// layout has the two kernels inverted and every event located on its class's shape besides.
inline void es_pack(int likelihood, const double* p, std::vector<double>& out) {
    const bool shape = likelihood == SMCMC_LIKE_EVENT_SHAPE;
    const EventForm f = event_form(likelihood);
    const size_t nev = (size_t)p[0], nbins = (size_t)p[1];
    const size_t stride = shape ? SMCMC_ESH_EVENT : SMCMC_ES_EVENT;
    const size_t events_at = shape ? (size_t)SMCMC_ESH_EVENTS(nbins) : (size_t)SMCMC_ES_HEADER + 3 * nbins;
    out.assign(events_at + stride * nev, 0.0);
    // the header: the exposure slot of the shape is 1, its SMCMC_ES_H_CUT is cutClose
    const double pi = 3.14159265358979323846;
    out[SMCMC_ES_H_NEVENTS] = p[0]; out[SMCMC_ES_H_NBINS] = p[1]; out[SMCMC_ES_H_XMIN] = p[2]; out[SMCMC_ES_H_XMAX] = p[3];
    out[SMCMC_ES_H_EXPOSURE] = shape ? 1.0 : p[4]; out[SMCMC_ES_H_CUT] = p[5];
    if (shape) out[SMCMC_ESH_H_CUT_VERY_CLOSE] = p[4];
    out[SMCMC_ES_H_TRUE_FAKES] = p[6]; out[SMCMC_ES_H_TRUE_EFF] = p[7];
    out[SMCMC_ES_H_TAN_FAKES] = std::tan(pi * (p[6] - 0.5));        // SystematicCorrection.H:94 (example3/ the same)
    out[SMCMC_ES_H_TAN_EFF] = std::tan(pi * (p[7] - 0.5));          // :106; example3/:110
    out[SMCMC_ES_H_RANGE] = p[3] - p[2];
    for (size_t i = 0; i < f.nh * nbins; ++i) out[SMCMC_ES_HEADER + i] = p[f.header + i];
    const double* kb = p + f.header + f.nh * nbins;
    const double* ks = kb + 121;
    const double* cb = nullptr;
    const double* cs = nullptr;
    if (shape) {
        std::vector<double> inv;
        esh_invert(kb, SMCMC_ESH_NB, inv);
        for (size_t i = 0; i < 121; ++i) out[SMCMC_ESH_KINV_B(nbins) + i] = inv[i];
        esh_invert(ks, SMCMC_ESH_NS, inv);
        for (size_t i = 0; i < 169; ++i) out[SMCMC_ESH_KINV_S(nbins) + i] = inv[i];
        double* c = out.data() + SMCMC_ESH_CENTRE_B(nbins);
        for (int i = 0; i < SMCMC_ESH_NB; ++i) c[i] = smcmc_esh_centre(p[8], p[9], SMCMC_ESH_NB, i);
        for (int i = 0; i < SMCMC_ESH_NS; ++i) c[SMCMC_ESH_NB + i] = smcmc_esh_centre(p[10], p[11], SMCMC_ESH_NS, i);
        cb = c;
        cs = c + SMCMC_ESH_NB;
    }
    const double* ev = kb + f.kernels;
    size_t nsig = 0;
    if (f.two_pass) {
        for (size_t e = 0; e < nev; ++e) nsig += (ev[6 * e + 1] > 0.0) ? 0 : 1;
        out[SMCMC_ES_H_NSIGNAL] = (double)nsig;
    }
    size_t at[2] = {0, nsig};                                       // the next packed slot of a signal / a background event
    for (size_t e = 0; e < nev; ++e) {
        const double* q = ev + 6 * e;
        const double mass = q[0], true_mass = q[4], true_sigma = q[5];
        const int bkg = q[1] > 0.0 ? 1 : 0;
        const double nominalLogMass = smcmc_log(true_mass);                            // :57; example3/:54
        double nominalLogSigma = smcmc_log(true_mass + true_sigma);                    // :58; :55
        nominalLogSigma = nominalLogSigma - nominalLogMass;                            // :59; :56
        const double logMass = smcmc_log(mass);                                        // :61; :58
        const double logSigma = (logMass - nominalLogMass) / nominalLogSigma;          // :62; :59
        double* d = out.data() + events_at + stride * (f.two_pass ? at[bkg]++ : e);
        d[0] = nominalLogMass;
        d[1] = logMass - nominalLogMass;
        d[2] = logSigma;
        d[3] = q[2];
        d[4] = (double)(2 * bkg + (q[3] > 0.0 ? 1 : 0));
        if (shape) {
            int k, clamped;
            double dx;
            if (bkg) smcmc_esh_locate(mass, p[8], p[9], SMCMC_ESH_NB, cb, &k, &dx, &clamped);     // :104, 120: the uncorrected mass
            else smcmc_esh_locate(mass, p[10], p[11], SMCMC_ESH_NS, cs, &k, &dx, &clamped);
            d[5] = (double)k;
            d[6] = dx;
            d[7] = (double)clamped;
        }
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

// SMCMC_LIKE_EVENT_TEMPLATE (shape false: point[9]) and SMCMC_LIKE_EVENT_SHAPE (point[31]) from the packed layout, NH = 3
// or 4 histograms: log L; hist (may be null): the expectation [NH][nbins] before the clamp; parts (may be null):
// S[NH][nbins], B[NH][nbins], IS, IB, ws, wb, and for the shape penalty(B), penalty(S), KinvB, KinvS.  The device kernels
// make this walk with these functions.
inline double es_two_pass_packed(bool shape, const double* pk, const double* point, double* hist, double* parts) {
    const int nev = (int)pk[SMCMC_ES_H_NEVENTS], nbins = (int)pk[SMCMC_ES_H_NBINS], nsig = (int)pk[SMCMC_ES_H_NSIGNAL];
    const int nh = shape ? 4 : 3, rows = nh * nbins, stride = shape ? SMCMC_ESH_EVENT : SMCMC_ES_EVENT;
    smcmc_es_scalars s;
    const double true_fakes = pk[SMCMC_ES_H_TRUE_FAKES], true_eff = pk[SMCMC_ES_H_TRUE_EFF];
    const double tan_fakes = pk[SMCMC_ES_H_TAN_FAKES], tan_eff = pk[SMCMC_ES_H_TAN_EFF];
    if (shape) smcmc_esh_point_scalars(point, true_fakes, true_eff, tan_fakes, tan_eff, &s);
    else smcmc_et_point_scalars(point, true_fakes, true_eff, tan_fakes, tan_eff, &s);
    double yb[SMCMC_ESH_NB] = {}, ys[SMCMC_ESH_NS] = {}, slb[SMCMC_ESH_NB] = {}, sls[SMCMC_ESH_NS] = {};     // (the shape's alone)
    if (shape) {
        const double* cb = pk + SMCMC_ESH_CENTRE_B(nbins);
        const double* cs = pk + SMCMC_ESH_CENTRE_S(nbins);
        for (int i = 0; i < SMCMC_ESH_NB; ++i) yb[i] = smcmc_esh_control_b(point, i);
        for (int i = 0; i < SMCMC_ESH_NS; ++i) ys[i] = smcmc_esh_control_s(point, i);
        for (int i = 0; i + 1 < SMCMC_ESH_NB; ++i) slb[i] = smcmc_esh_slope(yb[i], yb[i + 1], cb[i], cb[i + 1]);
        for (int i = 0; i + 1 < SMCMC_ESH_NS; ++i) sls[i] = smcmc_esh_slope(ys[i], ys[i + 1], cs[i], cs[i + 1]);
        slb[SMCMC_ESH_NB - 1] = sls[SMCMC_ESH_NS - 1] = 0.0;       // (a clamped event's: never read into a value)
    }
    std::vector<double> h((size_t)2 * rows, 0.0);                   // S, then B
    const double* ev = pk + (shape ? SMCMC_ESH_EVENTS(nbins) : SMCMC_ES_HEADER + rows);
    double integral[2], norm[2];
    for (int c = 0; c < 2; ++c) {
        double* hc = h.data() + (size_t)c * rows;
        const double* y = c ? yb : ys;
        const double* sl = c ? slb : sls;
        for (int e = c ? nsig : 0; e < (c ? nev : nsig); ++e) {
            const double* q = ev + (size_t)stride * e;
            const int cls = (int)q[4];
            int b;
            double w = s.weight[cls];
            if (shape) {
                const int k = (int)q[5];
                b = smcmc_esh_event_bin(q[0], q[1], q[2], q[3], cls >> 1, cls & 1, &s, nbins, pk[SMCMC_ES_H_XMIN], pk[SMCMC_ES_H_XMAX],
                                        pk[SMCMC_ES_H_RANGE], pk[SMCMC_ESH_H_CUT_VERY_CLOSE], pk[SMCMC_ES_H_CUT]);
                w = smcmc_esh_weight(w, smcmc_esh_shape(y[k], sl[k], q[6], q[7] != 0.0));
            } else {
                b = smcmc_es_event_bin(q[0], q[1], q[2], q[3], cls >> 1, cls & 1, &s, nbins, pk[SMCMC_ES_H_XMIN], pk[SMCMC_ES_H_XMAX],
                                       pk[SMCMC_ES_H_RANGE], pk[SMCMC_ES_H_CUT]);
            }
            if (b >= 0) hc[b] = hc[b] + w;
        }
        double sum[4];
        for (int k = 0; k < nh; ++k) {
            sum[k] = 0.0;
            for (int b = 0; b < nbins; ++b) sum[k] += hc[k * nbins + b];
        }
        integral[c] = smcmc_et_integral(sum, nh);
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
        double* t = parts + 2 * rows;
        t[0] = integral[0]; t[1] = integral[1]; t[2] = norm[0]; t[3] = norm[1];
    }
    if (!shape) return smcmc_et_penalties(logl, point[0], point[1], point[6], point[7], point[8]);
    const double pen_b = smcmc_esh_gp_penalty(yb, pk + SMCMC_ESH_KINV_B(nbins), SMCMC_ESH_NB);
    const double pen_s = smcmc_esh_gp_penalty(ys, pk + SMCMC_ESH_KINV_S(nbins), SMCMC_ESH_NS);
    if (parts) {
        double* t = parts + 2 * rows + 4;
        t[0] = pen_b; t[1] = pen_s;
        for (int i = 0; i < 121 + 169; ++i) t[2 + i] = pk[SMCMC_ESH_KINV_B(nbins) + i];
    }
    return smcmc_esh_penalties(logl, point, pen_b, pen_s);
}

}  // namespace smcmc
