/* smcmc_event_shape.h -- the arithmetic of SMCMC_LIKE_EVENT_SHAPE (include/smcmc.h states the definition), one copy
 * for the device kernels and for the host entry point smcmc_event_shape_evaluate: example3/SystematicCorrection.H,
 * example3/FakeLikelihood.H and TFakeGP.H of the reference restated on include/smcmc_detmath.h.  Included by
 * smcmc_event_sample.h, whose per-event layout, bin term, normalisation and bin expectation it shares
 * (smcmc_es_bin_term, smcmc_et_norm, smcmc_et_mc_signal, smcmc_et_mc).  Compile with -ffp-contract=off.
 *
 * The engine's own layout of the sample ("packed", made once on the host by smcmc::esh_pack):
 *   [0, 16)                 header, SMCMC_ES_H_* (the exposure slot is 1, SMCMC_ES_H_CUT is cutClose) and SMCMC_ESH_H_*
 *   [16, 16 + 4 nbins)      data: VeryClose, Close, Separated, DecayTag
 *   then 121, 169           KinvB[11][11], KinvS[13][13]: the two kernel matrices inverted, once, on the host
 *   then 11, 13             the centres of the background's and of the signal's control bins
 *   then nevents x 8        per event {log TrueMass, log Mass - log TrueMass, logSigma, Separation, class, k, dx, clamped},
 *                           the events partitioned by class, signal first (SMCMC_ES_H_NSIGNAL)
 * k, dx, clamped locate the event's uncorrected mass on its class's shape (smcmc_esh_locate): none depends on the point.
 */
#ifndef SMCMC_EVENT_SHAPE_H_SEEN
#define SMCMC_EVENT_SHAPE_H_SEEN

enum {
    SMCMC_ESH_H_CUT_VERY_CLOSE = 12,    /* header slot; SMCMC_ES_H_CUT holds cutClose */
    SMCMC_ESH_DIM = 31,
    SMCMC_ESH_NB = 11,                  /* control points of the background's shape: p[9 .. 19] */
    SMCMC_ESH_NS = 13,                  /* ... of the signal's: a fixed zero, p[20 .. 30], a fixed zero */
    SMCMC_ESH_EVENT = 8,                /* doubles per packed event */
    SMCMC_ESH_PARAM_HEADER = 12,        /* doubles in front of the data in the caller's array (smcmc.h) */
    SMCMC_ESH_TABLES = 121 + 169 + 11 + 13      /* doubles between the data and the events */
};
/* offsets into the packed layout, nbins the header's */
#define SMCMC_ESH_KINV_B(nbins) (SMCMC_ES_HEADER + 4 * (nbins))
#define SMCMC_ESH_KINV_S(nbins) (SMCMC_ESH_KINV_B(nbins) + 121)
#define SMCMC_ESH_CENTRE_B(nbins) (SMCMC_ESH_KINV_S(nbins) + 169)
#define SMCMC_ESH_CENTRE_S(nbins) (SMCMC_ESH_CENTRE_B(nbins) + 11)
#define SMCMC_ESH_EVENTS(nbins) (SMCMC_ES_HEADER + 4 * (nbins) + SMCMC_ESH_TABLES)

/* The point's scalars (example3/SystematicCorrection.H:11-26 gives the order): the mass and separation corrections are
 * example's with the new indices; the tag fractions take the parameter divided by ten inside the arctangent. */
SMCMC_HD void smcmc_esh_point_scalars(const double* p, double true_fakes, double true_eff, double tan_fakes, double tan_eff,
                                      smcmc_es_scalars* s) {
    const double pi = 3.14159265358979323846;                       /* M_PI */
    s->scale = p[6] / 10.0;                                          /* example3/SystematicCorrection.H:61 */
    s->width = smcmc_exp(p[7] / 10.0);                               /* :62 */
    s->skew = 0.3 * smcmc_erf(p[8] / 10.0);                          /* :65 */
    s->sep[0] = smcmc_exp(p[2] / 10.0);                              /* :38, 41 */
    s->sep[1] = smcmc_exp(p[3] / 10.0);                              /* :39, 41 */
    double cf = tan_fakes;                                           /* :94 */
    cf += p[4] / 10.0;                                               /* :95 */
    cf = smcmc_atan(cf) / pi + 0.5;                                  /* :96 */
    double ce = tan_eff;                                             /* :110 */
    ce += p[5] / 10.0;                                               /* :111 */
    ce = smcmc_atan(ce) / pi + 0.5;                                  /* :112 */
    s->weight[0] = (1.0 - cf) / (1.0 - true_fakes);                  /* :100 */
    s->weight[1] = cf / true_fakes;                                  /* :99 */
    s->weight[2] = (1.0 - ce) / (1.0 - true_eff);                    /* :116 */
    s->weight[3] = ce / true_eff;                                    /* :115 */
}

/* control value i of the background's shape, 0 <= i < 11 (:139-140) */
SMCMC_HD double smcmc_esh_control_b(const double* p, int i) { return p[9 + i] / 10.0; }
/* ... and of the signal's, 0 <= i < 13: the end points are never set and stay zero (:145-147, :156-161) */
SMCMC_HD double smcmc_esh_control_s(const double* p, int i) { return (i == 0 || i == 12) ? 0.0 : p[19 + i] / 10.0; }

/* TAxis::GetBinCenter of bin i (from 0) of n equal bins over [low, high] */
SMCMC_HD double smcmc_esh_centre(double low, double high, int n, int i) {
    const double bw = (high - low) / (double)n;
    return low + (double)i * bw + 0.5 * bw;
}

/* TH1::Interpolate's choice of a segment for x on control bins with centres c[0 .. n): *k the control value the line
 * starts at, *dx = x - c[k]; *clamped = 1 at or beyond the outer centres, where the value is y[*k] itself (*dx = 0). */
SMCMC_HD void smcmc_esh_locate(double x, double low, double high, int n, const double* c, int* k, double* dx, int* clamped) {
    *dx = 0.0;
    *clamped = 1;
    if (x <= c[0]) { *k = 0; return; }
    if (x >= c[n - 1]) { *k = n - 1; return; }
    int b = (int)(((double)n * (x - low)) / (high - low));
    if (b > n - 1) b = n - 1;
    int kk = (x <= c[b]) ? b - 1 : b;
    if (kk < 0) kk = 0;
    if (kk > n - 2) kk = n - 2;
    *k = kk;
    *dx = x - c[kk];
    *clamped = 0;
}

/* the slope of segment k: it depends on the point and not on the event */
SMCMC_HD double smcmc_esh_slope(double y0, double y1, double c0, double c1) { return (y1 - y0) / (c1 - c0); }

/* TFakeGP::GetValue from what smcmc_esh_locate left: y = y[k], slope = slope[k] (anything when clamped) */
SMCMC_HD double smcmc_esh_shape(double y, double slope, double dx, int clamped) { return clamped ? y : y + dx * slope; }

/* the weight of an event: its class's weight times exp(shape), one un-fused product (:104, 120) */
SMCMC_HD double smcmc_esh_weight(double class_weight, double shape) { return class_weight * smcmc_exp(shape); }

/* One event: its bin over the four histograms laid end to end (VeryClose 0 .. nbins - 1, Close, Separated, DecayTag), or
 * -1 when a cut or the axis drops it.  The mass and the separation are smcmc_es_event_bin's, line for line; the split is
 * example3/FakeLikelihood.H:265-300. */
SMCMC_HD int smcmc_esh_event_bin(double nlm, double dlm, double lsg, double sepn, int background, int tagged,
                                 const smcmc_es_scalars* s, int nbins, double xmin, double xmax, double range,
                                 double cut_very_close, double cut_close) {
    const double skew = smcmc_exp(lsg * s->skew);                    /* example3/SystematicCorrection.H:66 */
    double lm = nlm + dlm * skew;                                    /* :69 */
    lm = nlm + (lm - nlm) * s->width;                                /* :70 */
    lm = lm + s->scale;                                              /* :71 */
    const double mass = smcmc_exp(lm);                               /* :73 */
    const double sep = sepn * (background ? s->sep[1] : s->sep[0]);  /* :45 */
    if (mass > 500.0) return -1;                                     /* example3/FakeLikelihood.H:265 */
    if (mass < 0.0) return -1;                                       /* :266 */
    if (sep < 0.0) return -1;                                        /* :267 */
    const int hist = tagged ? 3 : (sep < cut_very_close) ? 0 : (sep < cut_close) ? 1 : 2;   /* :268-300 */
    if (!(mass >= xmin) || !(mass < xmax)) return -1;                /* under- and overflow, NaN */
    int b = (int)(((double)nbins * (mass - xmin)) / range);
    if (b > nbins - 1) b = nbins - 1;                                /* (the quotient rounded up to nbins) */
    return hist * nbins + b;
}

/* A class's integral from the sums of its four histograms over their bins, added in the order of
 * example3/FakeLikelihood.H:303-306: DecayTag, VeryClose, Close, Separated. */
SMCMC_HD double smcmc_esh_integral(double very_close, double close, double separated, double decay_tag) {
    double v = decay_tag;
    v += very_close;
    v += close;
    v += separated;
    return v;
}

/* one term of TFakeGP::GetPenalty (TFakeGP.H:140-141) */
SMCMC_HD double smcmc_esh_gp_term(double yi, double yj, double kinv_ij) { return (yi * yj) * kinv_ij; }
/* TFakeGP::GetPenalty (:137-145): y the n control values, kinv the inverse kernel, row-major; i outer, j inner, from +0
 * (the device kernels write the same two loops over their own address spaces) */
SMCMC_HD double smcmc_esh_gp_penalty(const double* y, const double* kinv, int n) {
    double penalty = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) penalty += smcmc_esh_gp_term(y[i], y[j], kinv[i * n + j]);
    return penalty;
}

/* the penalty terms on the bin sum (example3/FakeLikelihood.H:104-134), p the point */
SMCMC_HD double smcmc_esh_penalties(double logl, const double* p, double penalty_b, double penalty_s) {
    if (p[0] < 0.0) logl -= 10.0 + __builtin_fabs(logl);             /* :109 */
    if (p[1] < 0.0) logl -= 10.0 + __builtin_fabs(logl);             /* :113 */
    double v = p[3] / 5.0;                                           /* :117 */
    logl -= (0.5 * v) * v;
    v = p[4] / 1.0;                                                  /* :122 */
    logl -= (0.5 * v) * v;
    v = p[5] / 1.0;                                                  /* :127 */
    logl -= (0.5 * v) * v;
    logl -= penalty_b;                                               /* :130-131 */
    logl -= penalty_s;                                               /* :133-134 */
    return logl;
}

#endif
