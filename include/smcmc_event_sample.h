/* smcmc_event_sample.h -- the arithmetic of SMCMC_LIKE_EVENT_SAMPLE (include/smcmc.h states the definition), one
 * copy for the device kernels and for the host entry point smcmc_event_sample_evaluate: example/SystematicCorrection.H
 * and example/FakeLikelihood.H of the reference restated on include/smcmc_detmath.h, so that host and gfx950 give the
 * same bits.  Compile with -ffp-contract=off.
 *
 * The engine's own layout of the sample ("packed", made once on the host by smcmc::es_pack, smcmc_event_sample_host.hpp):
 *   [0, 16)               header, SMCMC_ES_H_*
 *   [16, 16 + 3 nbins)    data: Close, Separated, DecayTag
 *   then nevents x 6      per event {log TrueMass, log Mass - log TrueMass, logSigma, Separation, class, 0}
 * Everything of an event that does not depend on the point is in there already: nominalLogMass, the difference
 * logMass - nominalLogMass and its quotient by nominalLogSigma (SystematicCorrection.H:57-62).  class = 2 (Type > 0) +
 * 1 (MuDk > 0) picks one of four weights, which depend on the point alone.
 *
 * SMCMC_LIKE_EVENT_TEMPLATE (example2/ of the reference; smcmc.h states the definition) shares the layout, the per-event
 * part and the bin term; its own arithmetic -- the four weights, the class integral, the normalisation, the expectation
 * of a bin and the penalties -- is the smcmc_et_* functions below.  For it es_pack partitions the events by class, signal
 * first and otherwise in the caller's order, and writes the number of signal events to the header (SMCMC_ES_H_NSIGNAL): no
 * histogram takes events of both classes, so no sum's order of additions changes.
 *
 * SMCMC_LIKE_EVENT_SHAPE (example3/) has a layout and functions of its own, smcmc_event_shape.h, included below.
 */
#ifndef SMCMC_EVENT_SAMPLE_H_SEEN
#define SMCMC_EVENT_SAMPLE_H_SEEN

#include "smcmc_detmath.h"

enum {
    SMCMC_ES_H_NEVENTS = 0, SMCMC_ES_H_NBINS, SMCMC_ES_H_XMIN, SMCMC_ES_H_XMAX, SMCMC_ES_H_EXPOSURE, SMCMC_ES_H_CUT,
    SMCMC_ES_H_TRUE_FAKES, SMCMC_ES_H_TRUE_EFF, SMCMC_ES_H_TAN_FAKES, SMCMC_ES_H_TAN_EFF, SMCMC_ES_H_RANGE,
    SMCMC_ES_H_NSIGNAL,         /* EVENT_TEMPLATE: events [0, nsignal) are the signal's, the rest the background's */
    SMCMC_ES_HEADER = 16,       /* doubles in front of the data */
    SMCMC_ES_EVENT = 6,         /* doubles per packed event */
    SMCMC_ES_PARAM_HEADER = 8,  /* doubles in front of the data in the caller's array (smcmc.h) */
    SMCMC_ES_DIM = 9
};

/* what an evaluation takes from the point before it walks the events */
typedef struct {
    double scale, width, skew, sep[2];  /* mass shift, mass width, 0.3 erf(p4/10), separation scale by Type */
    double weight[4];                   /* by class */
} smcmc_es_scalars;

/* the part of the scalars that corrects an event's mass and separation (SystematicCorrection.H:40-43, 64-68) */
SMCMC_HD void smcmc_es_mass_scalars(const double* p, smcmc_es_scalars* s) {
    s->scale = p[2] / 10.0;                                          /* SystematicCorrection.H:64 */
    s->width = smcmc_exp(p[3] / 10.0);                               /* :65 */
    s->skew = 0.3 * smcmc_erf(p[4] / 10.0);                          /* :68 */
    s->sep[0] = smcmc_exp(p[5] / 10.0);                              /* :40, 43 */
    s->sep[1] = smcmc_exp(p[6] / 10.0);                              /* :41, 43 */
}

/* the corrected fake probability and decay-tag efficiency (:94-96, 106-108) */
SMCMC_HD void smcmc_es_tag_fractions(const double* p, double tan_fakes, double tan_eff, double* fakes, double* eff) {
    const double pi = 3.14159265358979323846;                       /* M_PI */
    double cf = tan_fakes;                                           /* :94 */
    cf += p[7];                                                      /* :95 */
    cf = smcmc_atan(cf) / pi + 0.5;                                  /* :96 */
    double ce = tan_eff;                                             /* :106 */
    ce += p[8];                                                      /* :107 */
    ce = smcmc_atan(ce) / pi + 0.5;                                  /* :108 */
    *fakes = cf;
    *eff = ce;
}

/* p: the point; the other arguments: the header's values of those names */
SMCMC_HD void smcmc_es_point_scalars(const double* p, double exposure, double true_fakes, double true_eff,
                                     double tan_fakes, double tan_eff, smcmc_es_scalars* s) {
    smcmc_es_mass_scalars(p, s);
    const double ws = smcmc_exp(p[0] / 10.0);                        /* :87 */
    const double wb = smcmc_exp(p[1] / 10.0);                        /* :88 */
    double cf, ce;
    smcmc_es_tag_fractions(p, tan_fakes, tan_eff, &cf, &ce);
    s->weight[0] = (ws * ((1.0 - cf) / (1.0 - true_fakes))) * exposure;   /* :100, 115 */
    s->weight[1] = (ws * (cf / true_fakes)) * exposure;                   /* :99, 115 */
    s->weight[2] = (wb * ((1.0 - ce) / (1.0 - true_eff))) * exposure;     /* :112, 115 */
    s->weight[3] = (wb * (ce / true_eff)) * exposure;                     /* :111, 115 */
}

/* One event: its bin over the three histograms laid end to end (Close 0 .. nbins - 1, Separated, DecayTag), or -1 when a
 * cut or the axis drops it.  nlm, dlm, lsg, sepn: the packed event; background = class >= 2, tagged = class & 1. */
SMCMC_HD int smcmc_es_event_bin(double nlm, double dlm, double lsg, double sepn, int background, int tagged,
                                const smcmc_es_scalars* s, int nbins, double xmin, double xmax, double range, double cut) {
    const double skew = smcmc_exp(lsg * s->skew);                    /* SystematicCorrection.H:69 */
    double lm = nlm + dlm * skew;                                    /* :72 */
    lm = nlm + (lm - nlm) * s->width;                                /* :73 */
    lm = lm + s->scale;                                              /* :74 */
    const double mass = smcmc_exp(lm);                               /* :76 */
    const double sep = sepn * (background ? s->sep[1] : s->sep[0]);  /* :47 */
    if (mass > 500.0) return -1;                                     /* FakeLikelihood.H:203 */
    if (mass < 0.0) return -1;                                       /* :204 */
    if (sep < 0.0) return -1;                                        /* :205 */
    const int hist = tagged ? 2 : (sep < cut) ? 0 : 1;               /* :206-214 */
    if (!(mass >= xmin) || !(mass < xmax)) return -1;                /* under- and overflow, NaN */
    int b = (int)(((double)nbins * (mass - xmin)) / range);
    if (b > nbins - 1) b = nbins - 1;                                /* (the quotient rounded up to nbins) */
    return hist * nbins + b;
}

/* one bin's term of the sum (FakeLikelihood.H:54-59) */
SMCMC_HD double smcmc_es_bin_term(double data, double mc) {
    if (mc < 0.001) mc = 0.001;
    double v = data - mc;
    if (data > 0.0) v += data * smcmc_log(mc / data);
    return v;
}

/* ---- SMCMC_LIKE_EVENT_TEMPLATE (example2/) ---- */

/* The scalars of example2/SystematicCorrection.H: the mass and separation corrections are example's line for line; the
 * weights (:76-115, WEIGHT_SIGNAL_ANYWAY undefined) carry neither exp(p[0] / 10) nor an exposure ratio. */
SMCMC_HD void smcmc_et_point_scalars(const double* p, double true_fakes, double true_eff, double tan_fakes, double tan_eff,
                                     smcmc_es_scalars* s) {
    smcmc_es_mass_scalars(p, s);
    double cf, ce;
    smcmc_es_tag_fractions(p, tan_fakes, tan_eff, &cf, &ce);
    s->weight[0] = (1.0 - cf) / (1.0 - true_fakes);                  /* example2/SystematicCorrection.H:99 */
    s->weight[1] = cf / true_fakes;                                  /* :98 */
    s->weight[2] = (1.0 - ce) / (1.0 - true_eff);                    /* :111 */
    s->weight[3] = ce / true_eff;                                    /* :110 */
}

/* A class's integral from the sums of its three histograms over their bins (each ascending, from +0), added in the
 * order of example2/FakeLikelihood.H:266-268: DecayTag, then Close, then Separated.  TH1::Integral restated: under- and
 * overflow -- the dropped events -- are in none of the three. */
SMCMC_HD double smcmc_et_integral(double close, double separated, double decay_tag) {
    double v = decay_tag;
    v += close;
    v += separated;
    return v;
}

/* the factor that makes a class's histograms integrate to the fitted count (:269-270, 276-277): one IEEE division; an
 * empty class gives +-inf or NaN and nothing here looks at it */
SMCMC_HD double smcmc_et_norm(double count, double integral) { return count / integral; }

/* the signal's share of a bin's expectation (:280 ..: TH1::Add into a histogram that was reset) */
SMCMC_HD double smcmc_et_mc_signal(double ws, double s) { return 0.0 + ws * s; }
/* ... and the bin's expectation, the background's share added to it */
SMCMC_HD double smcmc_et_mc(double signal_share, double wb, double b) { return signal_share + wb * b; }

/* the penalty terms on the bin sum (:91-115), p the point */
SMCMC_HD double smcmc_et_penalties(double logl, const double* p) {
    if (p[0] < 0.0) logl -= 10.0 + __builtin_fabs(logl);             /* :96 */
    if (p[1] < 0.0) logl -= 10.0 + __builtin_fabs(logl);             /* :100 */
    double v = p[6] / 5.0;                                           /* :104 */
    logl -= (0.5 * v) * v;
    v = p[7] / 1.0;                                                  /* :109 */
    logl -= (0.5 * v) * v;
    v = p[8] / 1.0;                                                  /* :114 */
    logl -= (0.5 * v) * v;
    return logl;
}

#include "smcmc_event_shape.h"   /* SMCMC_LIKE_EVENT_SHAPE (example3/): the smcmc_esh_* functions */

#endif
