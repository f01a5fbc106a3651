/* smcmc_event_sample.h -- the arithmetic of the likelihoods over a simulated event sample (include/smcmc.h states the
 * definitions), one copy for the device kernels and for the host entry points smcmc_event_*_evaluate: one family with
 * three members, the reference's example/, example2/ and example3/ (SystematicCorrection.H and FakeLikelihood.H of each)
 * restated on include/smcmc_detmath.h, so that host and gfx950 give the same bits.  Compile with -ffp-contract=off.
 *
 *   SMCMC_LIKE_EVENT_SAMPLE    example/    three histograms filled with weights that carry the exposure ratio
 *   SMCMC_LIKE_EVENT_TEMPLATE  example2/   the same events as signal and background templates, each normalised by its own
 *                                          integral to a fitted count; penalty terms
 *   SMCMC_LIKE_EVENT_SHAPE     example3/   a fourth histogram and two Gaussian-process shapes on the weights
 *
 * Each piece is stated once, with the lines of the three examples it restates, and the members differ only where the
 * examples do: which parameters feed the mass scalars, the tag fractions and the penalties (arguments), the choice of
 * histogram (smcmc_es_event_bin, smcmc_esh_event_bin), the weights (smcmc_es_point_scalars against
 * smcmc_et_class_weights).  What only example3/ has -- the shapes, their penalties, its own packed layout -- is
 * smcmc_event_shape.h, included below.
 *
 * The engine's own layout of the sample ("packed", made once on the host by smcmc::es_pack, smcmc_event_sample_host.hpp):
 *   [0, 16)               header, SMCMC_ES_H_*
 *   [16, 16 + 3 nbins)    data: Close, Separated, DecayTag
 *   then nevents x 6      per event {log TrueMass, log Mass - log TrueMass, logSigma, Separation, class, 0}
 * Everything of an event that does not depend on the point is in there already: nominalLogMass, the difference
 * logMass - nominalLogMass and its quotient by nominalLogSigma (SystematicCorrection.H:57-62).  class = 2 (Type > 0) +
 * 1 (MuDk > 0) picks one of four weights, which depend on the point alone.
 *
 * For the two-pass members (_TEMPLATE, _SHAPE) es_pack partitions the events by class, signal first and otherwise in the
 * caller's order, and writes the number of signal events to the header (SMCMC_ES_H_NSIGNAL): no histogram of theirs takes
 * events of both classes, so no sum's order of additions changes.
 */
#ifndef SMCMC_EVENT_SAMPLE_H_SEEN
#define SMCMC_EVENT_SAMPLE_H_SEEN

#include "smcmc_detmath.h"

enum {
    SMCMC_ES_H_NEVENTS = 0, SMCMC_ES_H_NBINS, SMCMC_ES_H_XMIN, SMCMC_ES_H_XMAX, SMCMC_ES_H_EXPOSURE, SMCMC_ES_H_CUT,
    SMCMC_ES_H_TRUE_FAKES, SMCMC_ES_H_TRUE_EFF, SMCMC_ES_H_TAN_FAKES, SMCMC_ES_H_TAN_EFF, SMCMC_ES_H_RANGE,
    SMCMC_ES_H_NSIGNAL,         /* EVENT_TEMPLATE, EVENT_SHAPE: events [0, nsignal) are the signal's, the rest the background's */
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

/* The part of the scalars that corrects an event's mass and separation, from the five parameters it reads: p[2 .. 6] of
 * example/ and example2/ (SystematicCorrection.H:40-43, 64-68; example2's is the same text), p[6], p[7], p[8], p[2], p[3]
 * of example3/ (:38-41, 61-65). */
SMCMC_HD void smcmc_es_mass_scalars(double scale, double width, double skew, double sep_signal, double sep_background,
                                    smcmc_es_scalars* s) {
    s->scale = scale / 10.0;                                         /* SystematicCorrection.H:64; example3/:61 */
    s->width = smcmc_exp(width / 10.0);                              /* :65; :62 */
    s->skew = 0.3 * smcmc_erf(skew / 10.0);                          /* :68; :65 */
    s->sep[0] = smcmc_exp(sep_signal / 10.0);                        /* :40, 43; :38, 41 */
    s->sep[1] = smcmc_exp(sep_background / 10.0);                    /* :41, 43; :39, 41 */
}

/* The corrected fake probability and decay-tag efficiency (:94-96, 106-108; example3/:94-96, 110-112).  The two shifts:
 * p[7], p[8] in example/ and example2/, p[4] / 10, p[5] / 10 in example3/. */
SMCMC_HD void smcmc_es_tag_fractions(double shift_fakes, double shift_eff, double tan_fakes, double tan_eff, double* fakes,
                                     double* eff) {
    const double pi = 3.14159265358979323846;                       /* M_PI */
    double cf = tan_fakes;                                           /* :94 */
    cf += shift_fakes;                                               /* :95 */
    cf = smcmc_atan(cf) / pi + 0.5;                                  /* :96 */
    double ce = tan_eff;                                             /* :106; example3/:110 */
    ce += shift_eff;                                                 /* :107; :111 */
    ce = smcmc_atan(ce) / pi + 0.5;                                  /* :108; :112 */
    *fakes = cf;
    *eff = ce;
}

/* SMCMC_LIKE_EVENT_SAMPLE's scalars.  p: the point; the other arguments: the header's values of those names */
SMCMC_HD void smcmc_es_point_scalars(const double* p, double exposure, double true_fakes, double true_eff,
                                     double tan_fakes, double tan_eff, smcmc_es_scalars* s) {
    smcmc_es_mass_scalars(p[2], p[3], p[4], p[5], p[6], s);
    const double ws = smcmc_exp(p[0] / 10.0);                        /* :87 */
    const double wb = smcmc_exp(p[1] / 10.0);                        /* :88 */
    double cf, ce;
    smcmc_es_tag_fractions(p[7], p[8], tan_fakes, tan_eff, &cf, &ce);
    s->weight[0] = (ws * ((1.0 - cf) / (1.0 - true_fakes))) * exposure;   /* :100, 115 */
    s->weight[1] = (ws * (cf / true_fakes)) * exposure;                   /* :99, 115 */
    s->weight[2] = (wb * ((1.0 - ce) / (1.0 - true_eff))) * exposure;     /* :112, 115 */
    s->weight[3] = (wb * (ce / true_eff)) * exposure;                     /* :111, 115 */
}

/* One event's corrected mass and separation (:69-76, 47; example3/:66-73, 45).  nlm, dlm, lsg, sepn: the packed event;
 * background = class >= 2. */
SMCMC_HD void smcmc_es_event_correct(double nlm, double dlm, double lsg, double sepn, int background,
                                     const smcmc_es_scalars* s, double* mass, double* sep) {
    const double skew = smcmc_exp(lsg * s->skew);                    /* SystematicCorrection.H:69; example3/:66 */
    double lm = nlm + dlm * skew;                                    /* :72; :69 */
    lm = nlm + (lm - nlm) * s->width;                                /* :73; :70 */
    lm = lm + s->scale;                                              /* :74; :71 */
    *mass = smcmc_exp(lm);                                           /* :76; :73 */
    *sep = sepn * (background ? s->sep[1] : s->sep[0]);              /* :47; :45 */
}

/* the three cuts on a corrected event (FakeLikelihood.H:203-205; example2/ the same; example3/FakeLikelihood.H:265-267):
 * nonzero when one of them drops it */
SMCMC_HD int smcmc_es_event_cut(double mass, double sep) {
    if (mass > 500.0) return 1;                                      /* FakeLikelihood.H:203; example3/:265 */
    if (mass < 0.0) return 1;                                        /* :204; :266 */
    if (sep < 0.0) return 1;                                         /* :205; :267 */
    return 0;
}

/* The axis rule (TH1::Fill): the bin of `mass` in histogram `hist` of the histograms laid end to end, or -1 for under- and
 * overflow. */
SMCMC_HD int smcmc_es_axis_bin(double mass, int hist, int nbins, double xmin, double xmax, double range) {
    if (!(mass >= xmin) || !(mass < xmax)) return -1;                /* under- and overflow, NaN */
    int b = (int)(((double)nbins * (mass - xmin)) / range);
    if (b > nbins - 1) b = nbins - 1;                                /* (the quotient rounded up to nbins) */
    return hist * nbins + b;
}

/* One event of example/ and example2/: its bin over the three histograms laid end to end (Close 0 .. nbins - 1,
 * Separated, DecayTag), or -1 when a cut or the axis drops it.  tagged = class & 1. */
SMCMC_HD int smcmc_es_event_bin(double nlm, double dlm, double lsg, double sepn, int background, int tagged,
                                const smcmc_es_scalars* s, int nbins, double xmin, double xmax, double range, double cut) {
    double mass, sep;
    smcmc_es_event_correct(nlm, dlm, lsg, sepn, background, s, &mass, &sep);
    if (smcmc_es_event_cut(mass, sep)) return -1;
    const int hist = tagged ? 2 : (sep < cut) ? 0 : 1;               /* :206-214 */
    return smcmc_es_axis_bin(mass, hist, nbins, xmin, xmax, range);
}

/* one bin's term of the sum (FakeLikelihood.H:54-59) */
SMCMC_HD double smcmc_es_bin_term(double data, double mc) {
    if (mc < 0.001) mc = 0.001;
    double v = data - mc;
    if (data > 0.0) v += data * smcmc_log(mc / data);
    return v;
}

/* ---- SMCMC_LIKE_EVENT_TEMPLATE (example2/) and what SMCMC_LIKE_EVENT_SHAPE (example3/) shares with it ---- */

/* The four class weights of example2/SystematicCorrection.H:98-111 and example3/SystematicCorrection.H:99-116
 * (WEIGHT_SIGNAL_ANYWAY undefined): neither exp(p[0] / 10) nor an exposure ratio. */
SMCMC_HD void smcmc_et_class_weights(double cf, double ce, double true_fakes, double true_eff, smcmc_es_scalars* s) {
    s->weight[0] = (1.0 - cf) / (1.0 - true_fakes);                  /* example2/SystematicCorrection.H:99; example3/:100 */
    s->weight[1] = cf / true_fakes;                                  /* :98; :99 */
    s->weight[2] = (1.0 - ce) / (1.0 - true_eff);                    /* :111; :116 */
    s->weight[3] = ce / true_eff;                                    /* :110; :115 */
}

/* The scalars of example2/SystematicCorrection.H: the mass and separation corrections are example's line for line. */
SMCMC_HD void smcmc_et_point_scalars(const double* p, double true_fakes, double true_eff, double tan_fakes, double tan_eff,
                                     smcmc_es_scalars* s) {
    smcmc_es_mass_scalars(p[2], p[3], p[4], p[5], p[6], s);
    double cf, ce;
    smcmc_es_tag_fractions(p[7], p[8], tan_fakes, tan_eff, &cf, &ce);
    smcmc_et_class_weights(cf, ce, true_fakes, true_eff, s);
}

/* A class's integral from the sums of its nh histograms over their bins (each ascending, from +0), added in the order of
 * example2/FakeLikelihood.H:266-268 and example3/FakeLikelihood.H:303-306: DecayTag -- the last --, then the others
 * ascending.  TH1::Integral restated: under- and overflow -- the dropped events -- are in none of them. */
SMCMC_HD double smcmc_et_integral(const double* sum, int nh) {
    double v = sum[nh - 1];
    for (int k = 0; k + 1 < nh; ++k) v += sum[k];
    return v;
}

/* the factor that makes a class's histograms integrate to the fitted count (:269-270, 276-277): one IEEE division; an
 * empty class gives +-inf or NaN and nothing here looks at it */
SMCMC_HD double smcmc_et_norm(double count, double integral) { return count / integral; }

/* the signal's share of a bin's expectation (:280 ..: TH1::Add into a histogram that was reset) */
SMCMC_HD double smcmc_et_mc_signal(double ws, double s) { return 0.0 + ws * s; }
/* ... and the bin's expectation, the background's share added to it */
SMCMC_HD double smcmc_et_mc(double signal_share, double wb, double b) { return signal_share + wb * b; }

/* The sign and Gaussian penalty terms on the bin sum (example2/FakeLikelihood.H:91-115, example3/FakeLikelihood.H:104-127)
 * over the five parameters they read: the two counts, then p[6], p[7], p[8] of example2/, p[3], p[4], p[5] of example3/. */
SMCMC_HD double smcmc_et_penalties(double logl, double count_s, double count_b, double sep_b, double fakes, double eff) {
    if (count_s < 0.0) logl -= 10.0 + __builtin_fabs(logl);          /* :96; example3/:109 */
    if (count_b < 0.0) logl -= 10.0 + __builtin_fabs(logl);          /* :100; :113 */
    double v = sep_b / 5.0;                                          /* :104; :117 */
    logl -= (0.5 * v) * v;
    v = fakes / 1.0;                                                 /* :109; :122 */
    logl -= (0.5 * v) * v;
    v = eff / 1.0;                                                   /* :114; :127 */
    logl -= (0.5 * v) * v;
    return logl;
}

#include "smcmc_event_shape.h"   /* SMCMC_LIKE_EVENT_SHAPE (example3/): the smcmc_esh_* functions */

#endif
