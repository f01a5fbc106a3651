/* smcmc_event_shape.h -- the arithmetic of SMCMC_LIKE_EVENT_SHAPE (include/smcmc.h states the definition), one copy
 * for the device kernels and for the host entry point smcmc_event_shape_evaluate: example3/SystematicCorrection.H,
 * example3/FakeLikelihood.H and TFakeGP.H of the reference restated on include/smcmc_detmath.h.  Included by
 * smcmc_event_sample.h, which states what the three likelihoods of the family share: here is only what example3/ adds
 * -- its indices into the point, the split into four histograms, the two shapes and their penalties.  Compile with
 * -ffp-contract=off.
 *
 * The engine's own layout of the sample ("packed", made once on the host by smcmc::es_pack):
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

/* The point's scalars (example3/SystematicCorrection.H:11-26 gives the order): the family's mass scalars, tag fractions
 * and class weights (smcmc_event_sample.h) on example3's indices; the tag fractions take the parameter divided by ten
 * inside the arctangent. */
SMCMC_HD void smcmc_esh_point_scalars(const double* p, double true_fakes, double true_eff, double tan_fakes, double tan_eff,
                                      smcmc_es_scalars* s) {
    smcmc_es_mass_scalars(p[6], p[7], p[8], p[2], p[3], s);
    double cf, ce;
    smcmc_es_tag_fractions(p[4] / 10.0, p[5] / 10.0, tan_fakes, tan_eff, &cf, &ce);
    smcmc_et_class_weights(cf, ce, true_fakes, true_eff, s);
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

/* One event of example3/: its bin over the four histograms laid end to end (VeryClose 0 .. nbins - 1, Close, Separated,
 * DecayTag), or -1.  smcmc_es_event_bin with the split of example3/FakeLikelihood.H:268-300. */
SMCMC_HD int smcmc_esh_event_bin(double nlm, double dlm, double lsg, double sepn, int background, int tagged,
                                 const smcmc_es_scalars* s, int nbins, double xmin, double xmax, double range,
                                 double cut_very_close, double cut_close) {
    double mass, sep;
    smcmc_es_event_correct(nlm, dlm, lsg, sepn, background, s, &mass, &sep);
    if (smcmc_es_event_cut(mass, sep)) return -1;
    const int hist = tagged ? 3 : (sep < cut_very_close) ? 0 : (sep < cut_close) ? 1 : 2;   /* :268-300 */
    return smcmc_es_axis_bin(mass, hist, nbins, xmin, xmax, range);
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

/* the penalty terms on the bin sum (example3/FakeLikelihood.H:104-134), p the point: the family's, then the two shapes' */
SMCMC_HD double smcmc_esh_penalties(double logl, const double* p, double penalty_b, double penalty_s) {
    logl = smcmc_et_penalties(logl, p[0], p[1], p[3], p[4], p[5]);
    logl -= penalty_b;                                               /* :130-131 */
    logl -= penalty_s;                                               /* :133-134 */
    return logl;
}

#endif
