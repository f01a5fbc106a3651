/* smcmc.h -- C ABI of the MI355X many-chain adaptive Metropolis engine.
 *
 * Drop-in boundary for ONE path of ClarkMcGrew/root-simple-mcmc: the
 * sMCMC::TSimpleMCMC<L, sMCMC::TProposeAdaptiveStep>::Step() loop.  The reference
 * exposes no FFI; its boundary is the C++ template surface of TSimpleMCMC.H:185-590
 * and the TProposeAdaptiveStep public methods (TSimpleMCMC.H:732-1003).  The
 * host-side mirror of that surface (include/TSimpleMCMC_amd.H and the Python
 * package root-simple-mcmc_amd/) is written on top of exactly these entry
 * points; each one names the reference member it stands behind.
 *
 * Conventions: every function returns an smcmc_status (0 = ok); no exception
 * crosses the ABI; vectors over chains are laid out [dim][chain] (chain index
 * fastest), host buffers are caller-owned, one engine per (device, stream),
 * calls on one engine are serialised by the caller.  Kernel launches are
 * asynchronous on the engine's stream; every smcmc_read_* / smcmc_get_* /
 * smcmc_apply_moments call synchronises that stream first.
 */
#ifndef SMCMC_H_SEEN
#define SMCMC_H_SEEN

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smcmc_engine smcmc_engine;

typedef enum {
    SMCMC_OK = 0,
    SMCMC_ERR_INVALID = 1,      /* std::invalid_argument in the reference (TSimpleMCMC.H:373,813,1153) */
    SMCMC_ERR_LOGIC = 2,        /* std::logic_error (TSimpleMCMC.H:666,673,1575) */
    SMCMC_ERR_RUNTIME = 3,      /* std::runtime_error (TSimpleMCMC.H:1027,1385,1479) */
    SMCMC_ERR_BAD_START = 4,    /* Start() returned false (TSimpleMCMC.H:265-268) */
    SMCMC_ERR_UNSUPPORTED = 5,  /* configuration the HIP path does not cover; never a CPU fallback */
    SMCMC_ERR_HIP = 6,          /* a HIP runtime call failed (smcmc_last_error has the text) */
    SMCMC_ERR_NO_DEVICE = 7
} smcmc_status;

/* Likelihood functors with a device implementation (the `UserLikelihood`
 * template argument of TSimpleMCMC.H:185). */
typedef enum {
    SMCMC_LIKE_ISO_GAUSS = 0,   /* README.md:57-66 / TSimpleMCMC.H:111-120: logL = sum -0.5 p_i^2 */
    SMCMC_LIKE_QUADFORM = 1,    /* TDummyLogLikelihood.H:21-31; params = Error matrix, dim*dim row-major */
    SMCMC_LIKE_ROSENBROCK = 2,  /* THardLogLikelihood.H:57-67; params = {ROSEN_B}, default 100 */
    /* A likelihood compiled in from user source (the `double operator()(const Vector&)` of the
     * reference's UserLikelihood concept, TSimpleMCMC.H:53-57, as a device function): a library built
     * with `python root-simple-mcmc_amd/build.py --user-likelihood my_likelihood.hip.h` carries it
     * (INTEGRATION.md); other builds answer SMCMC_ERR_UNSUPPORTED.  params = whatever the function reads (at most
     * dim_padded^2 doubles).  dim <= 63 with the register form (smcmc_user_loglike<DP>); a header that also defines
     * smcmc_user_loglike_at and SMCMC_USER_LIKELIHOOD_ANY_DIM is served up to dim = 512, above 63 in reference-order
     * arithmetic (SMCMC_P_EXACT_ARITHMETIC = 1).  Metropolis (smcmc_*) and variable-at-a-time (smcmc_vaat_*) engines. */
    SMCMC_LIKE_USER = 3,
    /* The reference's stress targets (Metropolis engine only; they have no gradient, TSimpleHMC.H:85-89):
     * TAsymLogLikelihood.H:20-31, params = {positiveSlope, negativeSlope} (default -1, 100);
     * THorrificLogLikelihood.H:26-38 (no parameters);
     * example4/TConstrainedLikelihood.H:26-46, params = {SummedValues, SummedConstraint, ExpectedValues[dim],
     * PriorConstraints[dim]}.
     * For dim > 63 all three run in reference-order arithmetic only. */
    SMCMC_LIKE_ASYM = 4,
    SMCMC_LIKE_HORRIFIC = 5,
    SMCMC_LIKE_CONSTRAINED = 6,
    /* example/FakeLikelihood.H: a binned Poisson likelihood over a simulated event sample, re-weighted and corrected by
     * nine systematic parameters (the definition follows below, "event sample").  dim = 9, Metropolis engine, frozen /
     * pooled / SMCMC_MODE_PER_CHAIN on the one-chain-per-wavefront kernel, reference-order arithmetic only. */
    SMCMC_LIKE_EVENT_SAMPLE = 7,
    /* example2/FakeLikelihood.H: the same analysis as a template fit -- the fitted parameters 0 and 1 are the signal and
     * background event counts, each class of the simulated sample is normalised by its own integral at every evaluation,
     * and penalty terms keep the corner cases in check (the definition follows below, "event template").  dim = 9; served
     * and refused exactly where SMCMC_LIKE_EVENT_SAMPLE is. */
    SMCMC_LIKE_EVENT_TEMPLATE = 8,
    /* example3/FakeLikelihood.H with TFakeGP.H: the template fit with a fourth histogram (VeryClose) and two shapes of
     * Gaussian-process control values that re-weight the background and the signal peak event by event, each with its
     * quadratic-form penalty (the definition follows below, "event shape").  dim = 31; served and refused exactly where
     * SMCMC_LIKE_EVENT_TEMPLATE is. */
    SMCMC_LIKE_EVENT_SHAPE = 9
} smcmc_likelihood;

/* ---- SMCMC_LIKE_EVENT_SAMPLE: the definition ------------------------------------------------------------------
 * The point is p[9], in the order of example/SystematicCorrection.H:11-22: SignalWeight, BackgroundWeight, MassScale,
 * MassWidth, MassSkew, SignalSeparationScale, BackgroundSeparationScale, FakeMuDkProb, MuDkEfficiency.
 *
 * smcmc_set_likelihood_params takes one flat array of 8 + 3 nbins + 6 nevents doubles:
 *   { nevents, nbins, xmin, xmax, exposureRatio, separationCut (100), trueFakes (0.05), trueEfficiency (0.5),
 *     data[3][nbins]      Close, Separated, DecayTag (FakeLikelihood.H:53-78 sums them in this order),
 *     events[nevents][6]  Mass, Type, Separation, MuDk, TrueMass, TrueMassSigma (Simulated.H:7-14);
 *                         Type 0 is signal, Type > 0 background; MuDk > 0 is a decay tag }
 * SMCMC_ERR_INVALID unless the count is exact, 1 <= nbins <= SMCMC_EVENT_SAMPLE_MAX_BINS, nevents >= 1, every field
 * finite, Mass, TrueMass and TrueMassSigma > 0, Type >= 0 (a data event, Type < 0, has no place in the simulated sample),
 * xmin < xmax, and trueFakes and trueEfficiency inside (0, 1).
 *
 * exp, log, erf, atan below are smcmc_exp, smcmc_log, smcmc_erf, smcmc_atan of smcmc_detmath.h; every other operation
 * is one IEEE operation, un-fused, in the order written.  The two tangents tan(pi (trueFakes - 0.5)) and
 * tan(pi (trueEfficiency - 0.5)) are constants of the sample: the host takes them from libm when it packs the parameters.
 *
 * Once per evaluation (SystematicCorrection.H):
 *   scale = p[2] / 10                                  :64      width = exp(p[3] / 10)                  :65
 *   skew  = 0.3 erf(p[4] / 10)                         :68
 *   sepS  = exp(p[5] / 10),  sepB = exp(p[6] / 10)     :40-43
 *   cf = atan(tanFakes + p[7]) / M_PI + 0.5            :94-96   ce = atan(tanEfficiency + p[8]) / M_PI + 0.5   :106-108
 *   weight of a signal event      (exp(p[0] / 10) * (MuDk > 0 ? cf / trueFakes : (1 - cf) / (1 - trueFakes))) * exposureRatio
 *   weight of a background event  (exp(p[1] / 10) * (MuDk > 0 ? ce / trueEfficiency : (1 - ce) / (1 - trueEfficiency))) * exposureRatio
 *                                                      :83-116
 * Per event, in the order of the array (CorrectEvent, :35-128):
 *   nominalLogMass = log(TrueMass);  nominalLogSigma = log(TrueMass + TrueMassSigma) - nominalLogMass       :57-59
 *   logMass = log(Mass);  logSigma = (logMass - nominalLogMass) / nominalLogSigma                           :61-62
 *       (none of the four depends on the point: the engine computes them once, on the host, with smcmc_log)
 *   logMass = nominalLogMass + (logMass - nominalLogMass) * exp(logSigma * skew)                            :69, 72
 *   logMass = nominalLogMass + (logMass - nominalLogMass) * width                                           :73
 *   logMass = logMass + scale;  mass = exp(logMass)                                                         :74, 76
 *   separation = Separation * (Type > 0 ? sepB : sepS)                                                      :47
 * The cuts and the split (FakeLikelihood.H:203-214): the event is dropped if mass > 500.0, if mass < 0.0 or if
 * separation < 0.0 (the reference's literals); it goes to DecayTag if MuDk > 0, else to Close if separation <
 * separationCut, else to Separated -- a separation equal to the cut is Separated.
 *   1. A bin's content is the sum of its events' weights in event order, one un-fused addition per event, from +0:
 *      the reference's Fill loop.  This is what makes a chain reproducible.
 *   2. The bin rule: for xmin <= mass < xmax, bin = int(nbins * (mass - xmin) / (xmax - xmin)) -- the product first,
 *      then one IEEE division, then truncation -- and a quotient that rounds up to nbins counts as nbins - 1.  Anything
 *      else is dropped, mass == xmax and a non-finite mass included.  TH1::Fill finds its bin through TAxis::FindBin;
 *      ROOT is absent where this was written and the rule is not pinned against it (as for smcmc_marginal_histograms).
 *   3. The bin sum (FakeLikelihood.H:53-78), over Close, then Separated, then DecayTag, bins ascending, from +0:
 *        mc = content;  if (mc < 0.001) mc = 0.001;
 *   4.   v = data - mc;  if (data > 0) v += data * log(mc / data);  logL += v
 *      with smcmc_log and one IEEE division.
 * Device and host (smcmc_event_sample_evaluate) compile this from one header, include/smcmc_event_sample.h. */
#define SMCMC_EVENT_SAMPLE_MAX_BINS 97   /* the largest nbins whose 3 nbins + 1 rows of 64 doubles fit one workgroup's LDS
                                          * (160 KiB) beside the step kernel's own (smcmc_kernels.hip.h derives and asserts it) */
/* The likelihood on the host, for what the reference does outside Step(): Init()'s exposure ratio (FakeLikelihood.H:
 * 107-143: evaluate at the origin with exposureRatio = 1, take data / mc from the histograms) and WriteSimulation()
 * (:173-179).  params / count as above, point[9]; *logl the log-likelihood, hist (may be NULL) the three simulated
 * histograms [3][nbins] at that point.  The same bits as the device.  It never steps a chain.  SMCMC_ERR_INVALID with
 * the parameter rules above (smcmc_event_sample_last_error has the text of the latest failure of the calling thread). */
int smcmc_event_sample_evaluate(const double* params, int count, const double* point, double* logl, double* hist);
const char* smcmc_event_sample_last_error(void);

/* ---- SMCMC_LIKE_EVENT_TEMPLATE: the definition ----------------------------------------------------------------
 * The point is p[9], in the order of example2/SystematicCorrection.H:11-22 (the names above); p[0] and p[1] are the
 * fitted numbers of signal and background events.
 *
 * The parameter array is SMCMC_LIKE_EVENT_SAMPLE's, field for field and rule for rule, and three rules more:
 * exposureRatio (slot 4) is exactly 1.0 (example2 has none), at least one event has Type 0 and at least one Type > 0.
 * Anything else is SMCMC_ERR_INVALID with a message.
 *
 * Once per evaluation: scale, width, skew, sepS, sepB, cf, ce as above (example2's mass and separation corrections are
 * example's line for line).  The event weights (example2/SystematicCorrection.H:76-115, WEIGHT_SIGNAL_ANYWAY undefined)
 * have no exp(p[0] / 10) factor and no exposure factor; 1.0 * w is w:
 *   signal, untagged      (1 - cf) / (1 - trueFakes)            signal, tagged      cf / trueFakes
 *   background, untagged  (1 - ce) / (1 - trueEfficiency)       background, tagged  ce / trueEfficiency
 * Per event: the corrected mass, the scaled separation, the cuts, the split into Close / Separated / DecayTag and the
 * bin rule are those above.
 *   1. Six histograms, S[3][nbins] from the Type 0 events and B[3][nbins] from the Type > 0 events; a bin's content is
 *      the sum of its events' weights in event order, un-fused, from +0 (example2/FakeLikelihood.H:232-264).
 *   2. IS = (sum DecayTagS + sum CloseS) + sum SeparatedS (:266-268): each of the three sums over the bins ascending, from
 *      +0, the three added in that order.  Under- and overflow -- the dropped events -- are not in it.  ws = p[0] / IS, one
 *      IEEE division (:269-270).  IB and wb = p[1] / IB likewise (:273-277).
 *   3. mc[h][b] = (0.0 + ws * S[h][b]) + wb * B[h][b] (:280-288): two products and an addition, un-fused.
 *   4. The bin sum: steps 3 and 4 above over Close, Separated, DecayTag with this mc (:64-89).
 *   5. The penalties, in this order (:91-115):
 *        if (p[0] < 0) logL -= 10.0 + fabs(logL);   then the same for p[1], on the logL just updated;
 *        v = p[6] / 5.0;  logL -= (0.5 * v) * v;    v = p[7] / 1.0;  logL -= (0.5 * v) * v;    v = p[8] / 1.0;  likewise.
 *   6. Nothing is special-cased: a class none of whose events survives at a point has IS == 0, ws is +-inf or NaN, mc is
 *      NaN and logL is NaN, on the host and on the device alike; the step's test rejects it as non-finite.
 * Steps 2 and 3 restate TH1::Integral and TH1::Add and are not pinned against ROOT (absent where this was written), as
 * the bin rule says of itself.
 * No histogram takes events of both types, so a stable partition of the events by Type, signal first, leaves every
 * sum's order of additions as it was: the engine packs the sample that way, and an interleaved array gives the bits of
 * the same events sorted.
 *
 * On the host: params / count as above, point[9]; *logl the log-likelihood, hist (may be NULL) mc[3][nbins] before the
 * clamp, parts (may be NULL) 6 nbins + 4 doubles: S[3][nbins], B[3][nbins], then IS, IB, ws, wb -- what
 * WriteSimulation and the tests of the intermediate stages need.  The same bits as the device; it never steps a chain.
 * smcmc_event_sample_last_error serves this entry point too. */
int smcmc_event_template_evaluate(const double* params, int count, const double* point, double* logl, double* hist,
                                  double* parts);

/* ---- SMCMC_LIKE_EVENT_SHAPE: the definition -------------------------------------------------------------------
 * Everything is SMCMC_LIKE_EVENT_TEMPLATE's but what follows.
 *
 * The point is p[31], in the order of example3/SystematicCorrection.H:11-26 (not example2's): 0 SignalWeight,
 * 1 BackgroundWeight, 2 SignalSeparationScale, 3 BackgroundSeparationScale, 4 FakeMuDkProb, 5 MuDkEfficiency, 6 MassScale,
 * 7 MassWidth, 8 MassSkew, 9 .. 19 BackgroundShape, 20 .. 30 SignalShape.
 *
 * The parameter array is 12 + 4 nbins + 121 + 169 + 6 nevents doubles:
 *   { nevents, nbins, xmin, xmax, cutVeryClose (50), cutClose (100), trueFakes, trueEfficiency,
 *     bkgLow (0), bkgHigh (500), sigLow (0), sigHigh (250),
 *     data[4][nbins]      VeryClose, Close, Separated, DecayTag (example3/FakeLikelihood.H:68-102 sums them in this order),
 *     KB[11][11], KS[13][13]   the two kernel matrices, what TFakeGP::SetKernel / GaussianKernel leave,
 *     events[nevents][6]  as above }
 * SMCMC_ERR_INVALID unless the count is exact, 1 <= nbins <= SMCMC_EVENT_SHAPE_MAX_BINS, and SMCMC_LIKE_EVENT_TEMPLATE's
 * rules hold where they apply (every field finite, Mass, TrueMass, TrueMassSigma > 0, Type >= 0, xmin < xmax, the two
 * fractions inside (0, 1), an event of either class), cutVeryClose <= cutClose, bkgLow < bkgHigh, sigLow < sigHigh, both
 * kernels exactly symmetric and the inversion below succeeds on both.
 *
 * When the parameters are set, once, on the host: KinvB and KinvS, TMatrixD::Invert (TFakeGP.H:132-136) restated as an LU
 * decomposition with partial pivoting and a forward and a back substitution per column of the inverse (smcmc::esh_invert;
 * not pinned against ROOT), on the kernel as given; the centres of the
 * control bins, centre(i) = low + i * bw + 0.5 * bw with bw = (high - low) / n (TAxis::GetBinCenter), n = 11 over
 * [bkgLow, bkgHigh] and n = 13 over [sigLow, sigHigh]; and for every event the segment of its class's shape that its
 * UNCORRECTED Mass x falls on (TH1::Interpolate; not pinned against ROOT, as the bin rule says of itself):
 *   x <= centre(0): the value is y[0];  x >= centre(n - 1): the value is y[n - 1] -- y[.] itself, never y + 0 * slope;
 *   otherwise b = int(n * (x - low) / (high - low)), k = b - 1 if x <= centre(b), else k = b, and the value is
 *   y[k] + (x - centre(k)) * ((y[k + 1] - y[k]) / (centre(k + 1) - centre(k))).
 *
 * Once per evaluation: scale = p[6] / 10, width = exp(p[7] / 10), skew = 0.3 erf(p[8] / 10), sepS = exp(p[2] / 10),
 * sepB = exp(p[3] / 10); cf = atan(tanFakes + p[4] / 10) / M_PI + 0.5 and ce = atan(tanEfficiency + p[5] / 10) / M_PI + 0.5
 * (example3/SystematicCorrection.H:94-96, 110-112: the parameter divided by ten); the four class weights from cf and ce
 * as above; the control values yB[i] = p[9 + i] / 10 (i < 11) and yS[0] = yS[12] = 0, yS[i + 1] = p[20 + i] / 10 (i < 11)
 * (:136-149); the slopes (y[k + 1] - y[k]) / (centre(k + 1) - centre(k)).
 * Per event: mass, separation and cuts as above; the weight is classWeight * exp(shape(Mass)), one un-fused product, the
 * signal's shape for Type 0 and the background's for Type > 0 (:98-121).  The event goes to DecayTag if MuDk > 0, else to
 * VeryClose if separation < cutVeryClose, else to Close if separation < cutClose, else to Separated
 * (example3/FakeLikelihood.H:268-300).
 *   1. Eight histograms, S[4][nbins] and B[4][nbins], in the order VeryClose, Close, Separated, DecayTag.
 *   2. IS = ((sum DecayTagS + sum VeryCloseS) + sum CloseS) + sum SeparatedS (:303-306); ws = p[0] / IS; IB, wb likewise.
 *   3. mc[h][b] = (0.0 + ws * S[h][b]) + wb * B[h][b].
 *   4. The bin sum over VeryClose, Close, Separated, DecayTag (:68-102).
 *   5. The penalties, in this order (:104-134): the two sign penalties on p[0] and p[1]; v = p[3] / 5.0, then p[4] / 1.0,
 *      then p[5] / 1.0, each logL -= (0.5 * v) * v; logL -= penalty(yB, KinvB); logL -= penalty(yS, KinvS), with
 *      penalty = sum_i sum_j (y[i] * y[j]) * Kinv(i, j), i outer, j inner, un-fused, from +0 (TFakeGP.H:137-145), over all
 *      11 and all 13 control values, the signal's fixed zeros included.
 *
 * On the host: params / count as above, point[31]; *logl the log-likelihood, hist (may be NULL) mc[4][nbins] before the
 * clamp, parts (may be NULL) 8 nbins + 6 + 121 + 169 doubles: S[4][nbins], B[4][nbins], IS, IB, ws, wb, penalty(B),
 * penalty(S), KinvB[121], KinvS[169].  The same bits as the device; it never steps a chain.
 * smcmc_event_sample_last_error serves this entry point too. */
#define SMCMC_EVENT_SHAPE_MAX_BINS 59   /* the largest nbins whose 4 nbins + 1 histogram rows and 25 table rows of 64 doubles
                                         * fit one workgroup's LDS beside the 31-wide step kernel's own (smcmc_kernels.hip.h
                                         * derives and asserts it) */
int smcmc_event_shape_evaluate(const double* params, int count, const double* point, double* logl, double* hist,
                               double* parts);
/* The two pieces of TFakeGP.H by themselves, for include/TFakeGP_amd.H and for tests; the arithmetic above, the same bits.
 * smcmc_event_shape_gp_value: TFakeGP::GetValue(x) on n >= 1 control values y over [low, high] (low < high).
 * smcmc_event_shape_gp_penalty: TFakeGP::GetPenalty for the n x n kernel (row-major, finite, exactly symmetric, n from 1
 * to 64) and the control values y; inverse (may be NULL) receives the n x n inverse the sum was taken with.
 * SMCMC_ERR_INVALID, with a message through smcmc_event_sample_last_error, when a rule is broken or the kernel cannot be
 * inverted. */
int smcmc_event_shape_gp_value(double low, double high, int n, const double* y, double x, double* value);
int smcmc_event_shape_gp_penalty(const double* kernel, int n, const double* y, double* penalty, double* inverse);

/* How the proposal covariance adapts over the ensemble. */
typedef enum {
    SMCMC_MODE_FROZEN = 0,  /* SetCovarianceFrozen(true) (TSimpleMCMC.H:937): every chain is an
                               independent reference chain on the shared, fixed decomposition */
    SMCMC_MODE_POOLED = 1,  /* running centre/covariance (TSimpleMCMC.H:1780-1820) pooled over all
                               chains through batch moments; UpdateProposal at every smcmc_sync */
    SMCMC_MODE_PER_CHAIN = 2 /* the reference's own mode, per chain: every chain keeps its own centre, covariance and
                               decomposition ([k][chain] columns in device memory), runs UpdateState every step
                               (:1721-1831, the covariance loop of :1795-1820 included) and UpdateProposal when its own
                               --fNextUpdate < 1 on an accepted step (:1824-1826).  Every chain is bit for bit the
                               reference chain on its random stream.  dim <= 63 (up to smcmc_max_perchain_dim() with
                               SMCMC_P_PERCHAIN_WORKGROUP = 1, up to smcmc_max_perchain_stream_dim() with
                               SMCMC_P_PERCHAIN_STREAM = 1, set first), reference-order arithmetic, Gaussian
                               proposals in every dimension; memory 12 dim (dim + 1) + 32 dim bytes per chain.
                               The shared getters (centre, covariance, decomposition, trials, trace) answer for
                               chain 0, the setters act on every chain; smcmc_read_chain_proposal reads any chain. */
} smcmc_mode;

/* Scalar knobs / observables of TProposeAdaptiveStep and TSimpleMCMC. */
typedef enum {
    SMCMC_P_COVARIANCE_WINDOW = 0,      /* Set/GetCovarianceWindow        TSimpleMCMC.H:914-915 */
    SMCMC_P_COVARIANCE_DEWEIGHT = 1,    /* SetCovarianceUpdateDeweighting :927 */
    SMCMC_P_ACCEPTANCE_WINDOW = 2,      /* Set/GetAcceptanceWindow        :982-983 */
    SMCMC_P_ACCEPTANCE_DEWEIGHT = 3,    /* SetAcceptanceUpdateDeweighting :987 */
    SMCMC_P_ACCEPTANCE_RIGIDITY = 4,    /* Set/GetAcceptanceRigidity      :1002-1003 (set: all chains) */
    SMCMC_P_TARGET_ACCEPTANCE = 5,      /* Set/GetTargetAcceptance        :977-978 */
    SMCMC_P_SIGMA = 6,                  /* Get/SetSigma                   :770,775 (set: all chains; get: chain 0) */
    SMCMC_P_MAXIMUM_CORRELATION = 7,    /* SetMaximumCorrelation          :909 */
    SMCMC_P_STEP_RMS_WINDOW = 8,        /* SetStepRMSWindow               :511 */
    SMCMC_P_NEXT_UPDATE = 9,            /* Set/GetNextUpdate              :992-993 (FROZEN: all chains) */
    SMCMC_P_COVARIANCE_TRIALS = 10,     /* Get/SetCovarianceTrials        :942,947 */
    SMCMC_P_CENTER_TRIALS = 11,         /* Get/SetEstimatedCenterTrials   :741,747 */
    SMCMC_P_COVARIANCE_TRACE = 12,      /* GetCovarianceTrace             :961 (read only) */
    SMCMC_P_TOTAL_STEPS = 13,           /* fTotalSteps                    :554 (read only) */
    SMCMC_P_SIGMA_TRACE = 14,           /* fSigmaTrace                    :1960 (read only) */
    SMCMC_P_UPDATE_COUNT = 15,          /* number of UpdateProposal calls (diagnostic, read only) */
    SMCMC_P_LAST_UPDATE_PATH = 16,      /* 0 Cholesky 1 conditioned 2 eigen 3 emergency 4 reset (read only) */
    SMCMC_P_EXACT_ARITHMETIC = 17,      /* 1: reference operation order (default); 0: fused multiply-add */
    SMCMC_P_MOMENT_STRIDE = 18,         /* POOLED, dim > 63: fold the current point into the pooled moments every n-th step (default 1) */
    SMCMC_P_MOMENT_GROUP = 19,          /* chains per moment group (read only: 64, or the slice size of the dim > 63 path) */
    SMCMC_P_KEEP_PROPOSED = 20,         /* 1: every launch leaves the proposal of its last step on the device for
                                           smcmc_read_proposed (fProposed / GetProposed, TSimpleMCMC.H:514, 576); default 0 */
    SMCMC_P_DEVICE_UPDATE = 21,         /* 1 (default): the pooled update (running centre / covariance, sigma rescale, Cholesky, operand
                                         * layouts) runs on the device with no host synchronisation; only a failed decomposition brings
                                         * the host's fallback ladder (TSimpleMCMC.H:1134-1389) in.  0: all of it on the host.  Same bits. */
    SMCMC_P_OVERLAP_UPDATE = 22,        /* 1: the next launch does not wait for the status of the update before it;
                                         * identical results unless that update falls back to the ladder, which then takes effect one
                                         * window late.  0 (default): parity mode */
    SMCMC_P_COVARIANCE_FROZEN = 23,     /* Set/GetCovarianceFrozen :937-938 inside SMCMC_MODE_PER_CHAIN: the covariance loop is
                                         * skipped, the centre still runs (SMCMC_MODE_FROZEN is the shared-decomposition form) */
    SMCMC_P_DENSE_QUADFORM = 24,        /* SMCMC_LIKE_QUADFORM: 1 = always the dense D^2-term sum.  0 (default): when the Error matrix is
                                         * sparse (at most a quarter of its entries non-zero, full diagonal, all finite) the serial sums
                                         * of the reference-order kernels and of SMCMC_MODE_PER_CHAIN walk its non-zero entries only --
                                         * bit for bit the dense sum (a skipped term is +-0), dense again for a non-finite point.
                                         * Reads back 1 whenever the dense sum is what runs. */
    SMCMC_P_PERCHAIN_WAVE = 25,         /* SMCMC_MODE_PER_CHAIN: which kernel steps the chains.  1: one chain per WAVEFRONT (the chain's
                                         * covariance in registers, its decomposition in LDS for a whole launch: the kernel for few
                                         * chains, down to the single chain of SimpleMCMC.C); 0: one chain per lane (its O(D^2) state
                                         * streamed through HBM every step); -1 (default): per wavefront.  Same images, same
                                         * bits either way.  Every built-in likelihood runs on both; SMCMC_LIKE_USER (a library
                                         * built with a user likelihood) on the per-wavefront kernel only, whatever is set
                                         * here.  Reads back what runs. */
    SMCMC_P_PERCHAIN_WORKGROUP = 26,    /* SMCMC_MODE_PER_CHAIN: 1 = one chain per WORKGROUP of 512 threads (the chain's covariance
                                         * and decomposition in registers for a whole launch), the kernel that serves
                                         * 1 <= dim <= smcmc_max_perchain_dim(); set it before smcmc_set_mode to ask for the mode
                                         * above dim 63 (the O(D^2) images of the mode are then D^2 doubles per chain and more).
                                         * 0 (default): the two kernels of SMCMC_P_PERCHAIN_WAVE, dim <= 63.  Same images, same
                                         * bits: at dim <= 63 the choice may change between launches; above 63 setting 0 again on a
                                         * per-chain engine is SMCMC_ERR_UNSUPPORTED.  Every built-in likelihood; SMCMC_LIKE_USER
                                         * when the user header defines SMCMC_USER_LIKELIHOOD_ANY_DIM.  Reads back 1 exactly when
                                         * this kernel is what runs (SMCMC_P_PERCHAIN_WAVE then reads back 0). */
    SMCMC_P_COUNT_ = 28,                /* the number of parameters.  It keeps its place in the text behind 26, where
                                         * tests/test_perchain_workgroup_cpu.py looks for it; parameters added since follow
                                         * it, and its value counts them. */
    SMCMC_P_PERCHAIN_STREAM = 27        /* SMCMC_MODE_PER_CHAIN: 1 = one chain per workgroup of 512 threads with the chain's
                                         * covariance and decomposition STREAMED from device memory, the kernel that serves
                                         * 63 < dim <= smcmc_max_perchain_stream_dim(); set it before smcmc_set_mode to ask for
                                         * the mode above smcmc_max_perchain_dim().  Opt-in like SMCMC_P_PERCHAIN_WORKGROUP, over
                                         * which it wins where both serve: the mode's images are 12 dim^2 bytes per chain, held
                                         * per started tile of 64 chains (at dim 512: 67 MB + 134 MB per tile, for one chain
                                         * too), plus 8 dim (dim + 1) bytes of working copies per chain.  At dim <= 63 it changes
                                         * nothing.  Same images, same bits.  Above smcmc_max_perchain_dim() setting 0 again on a
                                         * per-chain engine is SMCMC_ERR_UNSUPPORTED.  Likelihoods as SMCMC_P_PERCHAIN_WORKGROUP.
                                         * Reads back 1 exactly when this kernel is what runs (the two others then read 0). */
} smcmc_param;

/* Per-chain double fields (smcmc_read_lane_f64). */
typedef enum {
    SMCMC_LANE_LOGL = 0,            /* fAcceptedLogLikelihood  TSimpleMCMC.H:568 */
    SMCMC_LANE_SIGMA = 1,           /* fSigma                  :1955 */
    SMCMC_LANE_ACCEPTANCE = 2,      /* fAcceptance             :1934 */
    SMCMC_LANE_ACCEPTANCE_TRIALS = 3,
    SMCMC_LANE_RIGIDITY = 4,
    SMCMC_LANE_LAST_VALUE = 5,      /* fLastValue              :1838 */
    SMCMC_LANE_LAST_X0 = 6,         /* fLastPoint[0]           :1835 */
    SMCMC_LANE_STEP_RMS = 7,        /* fStepRMS                :580 */
    SMCMC_LANE_LOGL_PROPOSED = 8,   /* fProposedLogLikelihood  :589 */
    /* SMCMC_MODE_PER_CHAIN only */
    SMCMC_LANE_CENTER_TRIALS = 9,   /* fCentralPointTrials     :1849 */
    SMCMC_LANE_COVARIANCE_TRIALS = 10, /* fCovarianceTrials    :1867 */
    SMCMC_LANE_SIGMA_TRACE = 11,    /* fSigmaTrace             :1960 */
    SMCMC_LANE_F64_COUNT_
} smcmc_lane_f64;

/* Per-chain int32 fields (smcmc_read_lane_i32). */
typedef enum {
    SMCMC_LANE_TRIALS = 0,          /* fTrials      :1922 */
    SMCMC_LANE_SUCCESSES = 1,       /* fSuccesses   :1926 */
    SMCMC_LANE_NEXT_UPDATE = 2,     /* fNextUpdate  :1930 */
    SMCMC_LANE_NACCEPT = 3,         /* sum of Step() return values */
    SMCMC_LANE_STEP_RMS_TRIALS = 4, /* fStepRMSTrials :583 */
    SMCMC_LANE_LAST_ACCEPT = 5,     /* Step() return value of the latest step */
    /* SMCMC_MODE_PER_CHAIN only */
    SMCMC_LANE_UPDATE_STATUS = 6,   /* 0 between calls (inside a launch: a chain waiting for the host's fallback ladder) */
    SMCMC_LANE_DECOMP_FULL = 7,     /* 1: fDecomposition is a full matrix (the eigen rung of the ladder, :1252-1321) */
    SMCMC_LANE_CHAIN_STEPS = 8,     /* fTotalSteps :554 of the chain */
    SMCMC_LANE_UPDATE_COUNT = 9,    /* UpdateProposal calls of the chain (diagnostic) */
    SMCMC_LANE_LAST_UPDATE_PATH = 10, /* rung of the latest UpdateProposal: 0 Cholesky 1 conditioned 2 eigen 3 emergency 4 reset */
    SMCMC_LANE_I32_COUNT_
} smcmc_lane_i32;

/* ---- lifetime ---------------------------------------------------------- */
/* TSimpleMCMC constructor (TSimpleMCMC.H:203) + SetDim (:786).  chain_offset is the
 * global id of local chain 0 (the Philox stream of chain c is keyed on
 * chain_offset + c), so an ensemble sharded over ranks draws the same numbers as
 * the unsharded one.  Fails with SMCMC_ERR_NO_DEVICE when no GPU is visible. */
int smcmc_create(int dim, int nchains, int likelihood, uint64_t seed, uint32_t chain_offset,
                 int device, smcmc_engine** out);
int smcmc_destroy(smcmc_engine* h);
const char* smcmc_last_error(const smcmc_engine* h);
const char* smcmc_status_string(int status);
/* Build facts, callable without a GPU: library version, compiled kernel families. */
int smcmc_version(void);
int smcmc_max_register_dim(void);   /* largest dim of the register-resident kernels (63) */
int smcmc_max_dim(void);            /* largest dim any kernel covers (512) */
int smcmc_max_perchain_dim(void);   /* largest dim of SMCMC_MODE_PER_CHAIN without SMCMC_P_PERCHAIN_STREAM (SMCMC_P_PERCHAIN_WORKGROUP = 1) */
int smcmc_max_perchain_stream_dim(void);   /* largest dim of SMCMC_MODE_PER_CHAIN (SMCMC_P_PERCHAIN_STREAM = 1): smcmc_max_dim() */
/* hipStream_t to launch on (NULL = default stream). */
int smcmc_set_stream(smcmc_engine* h, void* hip_stream);

/* ---- configuration (before smcmc_start) -------------------------------- */
int smcmc_set_likelihood_params(smcmc_engine* h, const double* params, int count);   /* GetLogLikelihood() :239 */
int smcmc_set_mode(smcmc_engine* h, int mode);
int smcmc_set_gaussian(smcmc_engine* h, int dim, double sigma);                      /* SetGaussian :855 */
int smcmc_set_uniform(smcmc_engine* h, int dim, double minimum, double maximum);     /* SetUniform :833 */
/* SetScanDimension (TSimpleMCMC.H:820-830): while set, a step redraws only that dimension (about the
 * estimated centre, or uniformly) and leaves the proposal state alone; out of range = off. */
int smcmc_set_scan_dimension(smcmc_engine* h, int dim);
int smcmc_set_correlation(smcmc_engine* h, int dim1, int dim2, double correlation);  /* SetCorrelation :883 */
int smcmc_reset_correlations(smcmc_engine* h);                                       /* ResetCorrelations :874 */
int smcmc_set_param(smcmc_engine* h, int which, double value);
int smcmc_get_param(smcmc_engine* h, int which, double* value);

/* One entry of the reference's output tree (branches of TSimpleMCMC.H:208-215 and 1616-1626),
 * as SaveStep(true) writes it and Restore / RestoreState read it back (:282-352, :1501-1612). */
typedef struct smcmc_saved_state {
    double log_likelihood;              /* LogLikelihood */
    int32_t total_steps;                /* TotalSteps */
    double step_rms;                    /* StepRMS */
    int32_t trials;                     /* AdaptiveTrials */
    int32_t successes;                  /* AdaptiveSuccesses */
    int32_t next_update;                /* AdaptiveNextUpdate */
    double acceptance;                  /* AdaptiveAcceptance */
    double acceptance_trials;           /* AdaptiveAcceptanceTrials */
    double sigma;                       /* AdaptiveSigma */
    const double* central_point;        /* AdaptiveCentralPoint [dim] */
    double central_point_trials;        /* AdaptiveCentralPointTrials */
    const double* covariance;           /* AdaptiveCovariance: lower triangle, row major, dim (dim + 1) / 2 */
    double covariance_trials;           /* AdaptiveCovarianceTrials */
} smcmc_saved_state;
/* Restore(tree) (TSimpleMCMC.H:282-352, randomize = false) on a started engine: every chain
 * continues from `accepted` ([dim] broadcast or [dim][nchains]) with the saved state; the
 * likelihood is recomputed on the device and replaces the saved one when they differ by more
 * than 1E-4; the proposal is updated once (RestoreState, :1612). */
int smcmc_restore(smcmc_engine* h, const double* accepted, int broadcast, const smcmc_saved_state* state);

/* ---- the chain ---------------------------------------------------------- */
/* Start (TSimpleMCMC.H:246-276) + InitializeState (:1679-1714).  x0 is [dim] when
 * broadcast != 0, else [dim][nchains].  SMCMC_ERR_BAD_START when any chain's start
 * has a non-finite or < -0.999999E+10 log-likelihood. */
int smcmc_start(smcmc_engine* h, const double* x0, int broadcast);
/* nsteps x Step(save=false, metropolis) for every chain (TSimpleMCMC.H:370-496):
 * one kernel launch, state stays in registers between the steps. */
int smcmc_step(smcmc_engine* h, int nsteps, int metropolis);
/* Same, and after every `stride`-th step writes the accepted point and its
 * log-likelihood (the `Accepted` / `LogLikelihood` branches, TSimpleMCMC.H:208-210)
 * into caller-owned DEVICE buffers save_x[slot][dim_padded][nchains_padded] (rows
 * >= dim are zero), save_logl[slot][nchains_padded]; slots = nsteps / stride. */
/* nsteps x Step(false, metropolis) in one launch with a per-step record of one chain on the host: after every step
 * what TSimpleMCMC::Step() leaves in its members and SaveStep() reads -- records[step * smcmc_record_stride()]:
 * [0, dim) fAccepted, [dim, 2 dim) fProposed, [2 dim, 3 dim) the diagonal of the chain's covariance (GetCovarianceTrace,
 * TSimpleMCMC.H:961-967, is its sum in index order: the reader adds it up; SMCMC_REC_COVARIANCE_TRACE itself is 0), then
 * the scalars of smcmc_record_field.  SMCMC_MODE_PER_CHAIN with the
 * one-chain-per-wavefront kernel (SMCMC_P_PERCHAIN_WAVE) or a one-chain-per-workgroup kernel
 * (SMCMC_P_PERCHAIN_WORKGROUP, SMCMC_P_PERCHAIN_STREAM); SMCMC_ERR_UNSUPPORTED otherwise.  include/TSimpleMCMC_amd.H
 * runs Step() ahead with it (TSimpleMCMC.H:370-496 one call at a time is one launch and three read-backs per step). */
typedef enum {
    SMCMC_REC_LOGL = 0, SMCMC_REC_LOGL_PROPOSED, SMCMC_REC_STEP_RMS, SMCMC_REC_LAST_ACCEPT, SMCMC_REC_TRIALS,
    SMCMC_REC_SUCCESSES, SMCMC_REC_NEXT_UPDATE, SMCMC_REC_ACCEPTANCE, SMCMC_REC_ACCEPTANCE_TRIALS, SMCMC_REC_SIGMA,
    SMCMC_REC_CENTER_TRIALS, SMCMC_REC_COVARIANCE_TRIALS, SMCMC_REC_COVARIANCE_TRACE, SMCMC_REC_TOTAL_STEPS,
    SMCMC_REC_UPDATE_STATUS, SMCMC_REC_COUNT_
} smcmc_record_field;
/* smcmc_snapshot remembers the state of the whole ensemble on the device (points, per-chain scalars, every chain's
 * centre / covariance / decomposition, the step count); smcmc_rollback returns to it, any number of times.  Draws are
 * keyed on (chain, step), so stepping again from a snapshot repeats the same steps: TSimpleMCMC_amd.H's Step() runs
 * ahead of its caller with smcmc_step_recorded and takes the steps it ran too far back this way when a setter,
 * UpdateProposal() or SaveStep(true) needs the state AT the caller's step.  A started SMCMC_MODE_PER_CHAIN ensemble;
 * settings changed in between (smcmc_set_param ...) are not part of the snapshot. */
int smcmc_snapshot(smcmc_engine* h);
int smcmc_rollback(smcmc_engine* h);
int smcmc_record_stride(const smcmc_engine* h);      /* 3 dim + SMCMC_REC_COUNT_ */
int smcmc_step_recorded(smcmc_engine* h, int nsteps, int metropolis, int chain, double* records);
int smcmc_step_save(smcmc_engine* h, int nsteps, int metropolis, int stride,
                    double* save_x_device, double* save_logl_device);
/* ForceStep (TSimpleMCMC.H:811-817): the next step of every chain proposes
 * exactly `point` ([dim] broadcast or [dim][nchains]) without updating the
 * proposal state. */
int smcmc_force_step(smcmc_engine* h, const double* point, int broadcast);

/* ---- adaptation --------------------------------------------------------- */
/* Pooled covariance exchange, POOLED mode.  reduce: sum the per-wavefront moment
 * accumulators into the packed device vector M[(dim+1)(dim+2)/2] (row i <= dim,
 * col j <= i, row `dim` holding sum(y) and the point count) and clear them.
 * export/import copy M to/from a caller-owned DEVICE buffer so the caller can
 * all-reduce it over ranks (RCCL).  apply: running centre/covariance update fed
 * with the batch (TSimpleMCMC.H:1780-1820) and UpdateProposal (:1009-1390).
 * smcmc_sync = reduce + apply, the single-GPU form. */
int smcmc_reduce_moments(smcmc_engine* h);
int smcmc_moments_size(const smcmc_engine* h);
int smcmc_export_moments(smcmc_engine* h, double* dst_device);
int smcmc_import_moments(smcmc_engine* h, const double* src_device);
int smcmc_apply_moments(smcmc_engine* h);
int smcmc_sync(smcmc_engine* h);
/* Native exchange for callers without torch.distributed (the C++ mirror): one RCCL communicator per engine,
 * one rank per GPU.  Rank 0 makes the id (SMCMC_COMM_ID_BYTES bytes, an ncclUniqueId) and hands it to the
 * other ranks by its own means (file, socket, MPI); every rank then calls smcmc_comm_init, which blocks until
 * all nranks have arrived.  With a communicator attached smcmc_sync is reduce + ncclAllReduce(sum, f64) of M
 * on the engine's stream + apply (the one collective of the path), and
 * smcmc_allreduce_moments is the middle step on its own.  RCCL is loaded at the first call (dlopen), so the
 * library has no link-time dependency on it; SMCMC_ERR_UNSUPPORTED when it cannot be loaded. */
#define SMCMC_COMM_ID_BYTES 128
int smcmc_comm_unique_id(void* id_out);
int smcmc_comm_init(smcmc_engine* h, const void* id, int rank, int nranks);
int smcmc_comm_destroy(smcmc_engine* h);
int smcmc_comm_ranks(smcmc_engine* h);         /* ncclCommCount of the attached communicator; 0 without one, < 0 on error */
int smcmc_allreduce_moments(smcmc_engine* h);
int smcmc_update_proposal(smcmc_engine* h);   /* UpdateProposal() :1009 on the shared proposal */
int smcmc_reset_proposal(smcmc_engine* h);    /* ResetProposal()  :1396 */

/* ---- read back ---------------------------------------------------------- */
int smcmc_nchains_padded(const smcmc_engine* h);          /* nchains rounded up to 64 */
int smcmc_dim_padded(const smcmc_engine* h);              /* rows of the device state: the kernel family's register-array size */
int smcmc_read_state(smcmc_engine* h, double* x, double* logl);   /* GetAccepted :502, x[dim][nchains] */
/* GetProposed :514, x[dim][nchains]: the point the latest step proposed (after Start / Restore: the start point).
 * Needs SMCMC_P_KEEP_PROPOSED = 1 (SMCMC_ERR_LOGIC otherwise). */
int smcmc_read_proposed(smcmc_engine* h, double* x);
int smcmc_read_lane_f64(smcmc_engine* h, int field, double* out);
int smcmc_read_lane_i32(smcmc_engine* h, int field, int32_t* out);
int smcmc_read_moments(smcmc_engine* h, double* out);     /* host copy of M */
int smcmc_get_center(smcmc_engine* h, double* out);       /* GetEstimatedCenter :732 */
int smcmc_set_center(smcmc_engine* h, const double* in);  /* SetEstimatedCenter :733 */
int smcmc_get_covariance(smcmc_engine* h, double* out);   /* fCurrentCov, dim*dim */
int smcmc_set_covariance(smcmc_engine* h, const double* in);
int smcmc_get_decomposition(smcmc_engine* h, double* out);/* fDecomposition, dim*dim */
/* One chain's members, as the host mirror of the reference class keeps them for chain 0 after every Step(): any
 * pointer may be NULL.  x[dim] = fAccepted; proposed[dim] = fProposed (needs SMCMC_P_KEEP_PROPOSED outside
 * SMCMC_MODE_PER_CHAIN, which always keeps it); lanes_f64[SMCMC_LANE_F64_COUNT_], lanes_i32[SMCMC_LANE_I32_COUNT_]. */
int smcmc_read_chain(smcmc_engine* h, int chain, double* x, double* proposed, double* lanes_f64, int32_t* lanes_i32);
/* SMCMC_MODE_PER_CHAIN: the adaptive state of one chain -- fCentralPoint [dim], fCurrentCov [dim*dim],
 * fDecomposition [dim*dim] (TSimpleMCMC.H:1841-1893); any pointer may be NULL.  In the other modes the shared
 * proposal's (the same for every chain). */
int smcmc_read_chain_proposal(smcmc_engine* h, int chain, double* centre, double* covariance, double* decomposition);
/* device pointers for zero-copy consumers (x: [dim_padded][nchains_padded], logl: [nchains_padded]) */
int smcmc_state_device_ptr(smcmc_engine* h, double** x, double** logl);

/* Development aid: a device buffer of smcmc_nchains_padded() / 64 * 7 * 64 unsigned 64-bit words, zeroed by the caller, to
 * which a library built with -DSMCMC_STEP_PROFILE (tools/micro/build_stepprof.sh) adds the cycles its step kernel spent per
 * section (tools/micro/stepprof.py reads it).  The shipped library takes no stamps and never touches the buffer.  NULL
 * (the default) turns it off; the buffer must outlive every later step launch. */
int smcmc_set_step_profile(smcmc_engine* h, void* device_buffer);

/* ---- Hamiltonian Monte Carlo (sMCMC::TSimpleHMC, reference TSimpleHMC.H:119-973) ------ */
/* Every chain is a TSimpleHMC chain with the analytic gradient of the device likelihood.
 * SetMeanEpsilon(negative value) keeps |epsilon| fixed (every update of fMeanEpsilon is
 * guarded by fMeanEpsilon > 0, TSimpleHMC.H:304-343, 833-846) and SetLeapFrog(n) fixes the
 * leapfrog count (:190, 302): with both the chains are independent and a launch runs many
 * steps.  Otherwise (the reference's default) the chains retune themselves, see
 * smcmc_hmc_set_sync_interval.
 * Per-chain columns reuse smcmc_lane_f64 / smcmc_lane_i32: LOGL = -fAcceptedPotential,
 * LOGL_PROPOSED = -fProposedPotential, ACCEPTANCE = fCurrentAcceptance, TRIALS = fStepCount,
 * NACCEPT, LAST_ACCEPT, and the SMCMC_HMC_LANE_* aliases below. */
#define SMCMC_HMC_LANE_MEAN_EPSILON SMCMC_LANE_SIGMA          /* f64: fMeanEpsilon  (TSimpleHMC.H:888) */
#define SMCMC_HMC_LANE_REVERSAL_LEN SMCMC_LANE_RIGIDITY       /* f64: fReversalLen  (:894) */
#define SMCMC_HMC_LANE_LEAPFROG SMCMC_LANE_NEXT_UPDATE        /* i32: fLeapFrogSteps (:891) */
#define SMCMC_HMC_LANE_CONTRIBUTES SMCMC_LANE_SUCCESSES       /* i32: the latest step fed UpdateCovariance (:336) */
typedef struct smcmc_hmc smcmc_hmc;
int smcmc_hmc_create(int dim, int nchains, int likelihood, uint64_t seed, uint32_t chain_offset, int device,
                     smcmc_hmc** out);                                   /* TSimpleHMC ctor :130 */
int smcmc_hmc_destroy(smcmc_hmc* h);
const char* smcmc_hmc_last_error(const smcmc_hmc* h);
int smcmc_hmc_set_stream(smcmc_hmc* h, void* hip_stream);
int smcmc_hmc_set_likelihood_params(smcmc_hmc* h, const double* params, int count);   /* GetLogLikelihood :157 */
int smcmc_hmc_set_alpha(smcmc_hmc* h, double alpha);                     /* SetAlpha :175 */
/* 1 (default): the reference's operation order throughout.  0: the gradient of the quadratic-form
 * likelihood (TDummyLogLikelihood.H:34-42) sums its terms in the same order with one fused multiply-add
 * each, on the FP64 matrix pipe (dim <= 512); nothing else changes.  Before smcmc_hmc_start. */
int smcmc_hmc_set_exact_arithmetic(smcmc_hmc* h, int exact);
int smcmc_hmc_set_mean_epsilon(smcmc_hmc* h, double epsilon);            /* SetMeanEpsilon :181 (after Start, which resets it to 0.05) */
int smcmc_hmc_get_mean_epsilon(smcmc_hmc* h, double* epsilon);           /* GetMeanEpsilon :184 */
int smcmc_hmc_set_leapfrog(smcmc_hmc* h, int steps);                     /* SetLeapFrog :190 */
int smcmc_hmc_get_leapfrog(smcmc_hmc* h, int* steps);                   /* fLeapFrogSteps of chain 0, signed as :190 keeps it */
/* The covariance-driven tuning (UpdateCovariance :665-695, UpdateErrorMatrix :703-858) is pooled over the ensemble:
 * every chain folds the point it stood on into moment groups of smcmc_hmc_moment_group() chains each step, and every
 * `steps` steps (default 1) the pooled running covariance is brought up to date and UpdateErrorMatrix runs once; when
 * it goes through, every chain takes the new step length and leapfrog count (:833-847).  One chain and an interval of
 * one step is the reference chain.  Runs whenever the step length or the leapfrog count is not fixed;
 * smcmc_hmc_set_track_covariance(h, 1) keeps it running for a fixed step too (the Trace / Orbit outputs). */
int smcmc_hmc_set_sync_interval(smcmc_hmc* h, int steps);
/* Step(save, gradientType), TSimpleHMC.H:279 / PotentialGradient :467-532.  0, 1, 4: the likelihood's own gradient;
 * 2: CovariantGradient (:447-454) from the pooled running covariance (tracked from then on); 3: FiniteDifferenceGradient
 * (:417-444); 5: zero.  Types 2, 3, 5 need reference-order arithmetic (SMCMC_ERR_UNSUPPORTED otherwise). */
int smcmc_hmc_set_gradient_type(smcmc_hmc* h, int type);
int smcmc_hmc_get_gradient_type(const smcmc_hmc* h);
/* The caller's own gradient (the OptionalGradient argument of TSimpleHMC<UserLikelihood, OptionalGradient>, TSimpleHMC.H:79-89,
 * 119-128; BadGrad.C is the reference's driver).  HMC stays correct with a wrong gradient as long as the leapfrog is
 * reversible (:101-108), so the gradient of types 0 / 1 / 4 need not be the gradient of the likelihood.  Two ways:
 *  - compiled in: a user likelihood header (SMCMC_LIKE_USER, build.py --user-likelihood) that also defines
 *        #define SMCMC_USER_GRADIENT 1
 *        template <class Point> __device__ double smcmc_user_gradient_at(const Point& p, const double* params, int D, int i);
 *    returns component i of grad log L at p (what the reference functor writes to g[i]; the engine negates it, :486).
 *    It needs SMCMC_USER_LIKELIHOOD_ANY_DIM (the build fails otherwise) and runs in reference-order arithmetic.  Whether a
 *    library has a gradient is fixed when it is compiled: a gradient that declines per call (the bool the reference's
 *    functor returns, :87) is not supported.  The HMC engine takes up to 2 dim^2 + 2 dim + 8 user parameters, so that the
 *    likelihood and the gradient can each carry a matrix (examples/user_likelihood_quadgrad.hip.h).
 *  - at run time, for SMCMC_LIKE_QUADFORM: smcmc_hmc_set_gradient_matrix(h, G, dim*dim) makes types 0 / 1 / 4 compute
 *    g_i = -sum_j G(i,j) q_j (j ascending) while the potential stays 1/2 sum_i q_i (Error q)_i, which costs one more
 *    contraction per step.  (NULL, 0) clears it.  It takes effect at the next step, before or after Start.  Any other
 *    likelihood is SMCMC_ERR_INVALID; the fused order (smcmc_hmc_set_exact_arithmetic(h, 0)) is SMCMC_ERR_UNSUPPORTED,
 *    whichever of the two is set first.  Types 2 / 3 / 5 are unaffected.
 * smcmc_hmc_has_gradient: 1 when types 0 / 1 / 4 are served (ISO_GAUSS, QUADFORM, ROSENBROCK, a user library with a
 * gradient), 0 when they are SMCMC_ERR_RUNTIME (the stress targets, a user library without one; NULL). */
int smcmc_hmc_has_gradient(const smcmc_hmc* h);
int smcmc_hmc_set_gradient_matrix(smcmc_hmc* h, const double* G, int count);
int smcmc_hmc_set_track_covariance(smcmc_hmc* h, int on);
int smcmc_hmc_moment_group(const smcmc_hmc* h);
int smcmc_hmc_sync(smcmc_hmc* h);                                        /* the pooled update now (end of a run) */
/* The same in pieces, so that an ensemble sharded over engines / ranks pools its covariance as the Metropolis engine's does:
 * reduce (the moment groups of the steps since the last update summed into the packed device vector M[(dim+1)(dim+2)/2]:
 * sum x x^T by rows j <= i, then sum x and the number of points), export / import (copy M to / from a caller-owned DEVICE
 * buffer: the caller adds the ranks' vectors, e.g. one RCCL all-reduce), apply (UpdateCovariance fed with the batch, then
 * UpdateErrorMatrix, the same on every rank).  Set the sync interval beyond the steps of a window and call these at its
 * end; smcmc_hmc_sync = reduce + apply. */
/* (one reduction at a time: a second reduce -- explicit, or the sync a step triggers when the interval runs out --
 * before the apply of the first is SMCMC_ERR_LOGIC; a sharded run sets the interval beyond its window and syncs itself) */
int smcmc_hmc_moments_size(const smcmc_hmc* h);
int smcmc_hmc_reduce_moments(smcmc_hmc* h);
int smcmc_hmc_export_moments(smcmc_hmc* h, double* dst_device);
int smcmc_hmc_import_moments(smcmc_hmc* h, const double* src_device);
int smcmc_hmc_apply_moments(smcmc_hmc* h);
/* out[10]: fCurrentCovarianceTrace, fEstimatedOrbitLength, updates that went through, fCovarianceTrials,
 * fAveragePointTrials, fStepsRemaining, fStepsSinceUpdate, max scale, min scale, fEstimatedCovarianceTrace */
int smcmc_hmc_get_tuning(smcmc_hmc* h, double* out);
int smcmc_hmc_get_average_point(smcmc_hmc* h, double* out);              /* fAveragePoint [dim] */
int smcmc_hmc_get_covariance(smcmc_hmc* h, double* out);                 /* GetEstimatedCovariance :197, dim*dim */
int smcmc_hmc_start(smcmc_hmc* h, const double* x0, int broadcast);      /* Start :210-269 */
int smcmc_hmc_step(smcmc_hmc* h, int nsteps);                            /* nsteps x Step(false) :279-401 */
int smcmc_hmc_read_state(smcmc_hmc* h, double* q, double* momentum, double* logl);   /* fAccepted, fAcceptedMomentum */
/* fAccepted of every chain into a DEVICE buffer [dim][smcmc_hmc_nchains_padded] (one slot of a trace for
 * smcmc_autocorrelation_sums), on the engine's stream: what SimpleHMC.C:51-66 fills its tree with, without the trip to the host. */
int smcmc_hmc_copy_positions(smcmc_hmc* h, double* dst_device);
/* smcmc_hmc_step(h, nsteps) that leaves its trace on the device: the same chain bit for bit (state, lanes, tuning and
 * draws, in every mode and gradient type), and after every `stride`-th step of the call fAccepted of every live chain
 * goes into save_x[slot][dim][smcmc_hmc_nchains_padded] (the layout smcmc_hmc_copy_positions fills and the posterior
 * reducers read) and SMCMC_LANE_LOGL into save_logl[slot][smcmc_hmc_nchains_padded] (may be NULL), both caller-owned
 * DEVICE buffers.  SMCMC_LANE_LOGL is -fAcceptedPotential, the log-likelihood for the likelihoods here; the reference's
 * `LogLikelihood` branch of the HMC tree (TSimpleHMC.H:140) holds the potential itself, the other sign.
 * slots = nsteps / stride, counted from the start of each call; steps past the last slot still run.  Lanes >= nchains
 * and anything beyond slot slots - 1 are never written.  The stores sit in the step kernels beside the commit of
 * fAccepted, in instantiations of their own (smcmc_hmc_step runs the code it ran before): with a fixed step length and
 * leapfrog count (nothing tracked) the call is still one launch; the tuned modes keep their one step per launch.
 * (Gradient types 2 / 3 / 5 and the two- and four-tile matrix kernels of the quadratic form, 128 < dim <= 512, are
 * served by cutting the launch at the save steps and copying the slot on the device: the same bits.)  Work goes on the
 * engine's stream; nothing waits on the host where smcmc_hmc_step does not.  SMCMC_ERR_INVALID, with nothing launched
 * and nothing written: NULL handle, not started, save_x_device NULL, stride < 1, nsteps < 0. */
int smcmc_hmc_step_save(smcmc_hmc* h, int nsteps, int stride, double* save_x_device, double* save_logl_device);
int smcmc_hmc_nchains_padded(const smcmc_hmc* h);
int smcmc_hmc_read_lane_f64(smcmc_hmc* h, int field, double* out);
int smcmc_hmc_read_lane_i32(smcmc_hmc* h, int field, int32_t* out);
/* SMCMC_MODE_POOLED (default): the covariance-driven tuning pooled over the ensemble, as above.  SMCMC_MODE_PER_CHAIN:
 * every chain keeps its own fAveragePoint / fEstimatedCovariance and runs UpdateCovariance + UpdateErrorMatrix
 * (:665-858) after each of its steps, whatever is fixed (with a fixed step and count only the Trace / Orbit outputs
 * move), on the device: chain c is, bit for bit, the reference chain on the stream (seed, chain_offset + c), and
 * smcmc_hmc_step enqueues its steps without waiting on the device.  In that mode the sync interval and
 * set_track_covariance have no effect, smcmc_hmc_sync is a no-op, reduce / export / import / apply_moments are
 * SMCMC_ERR_LOGIC (nothing is pooled: shard by chain_offset), get_tuning / get_average_point / get_covariance report
 * chain 0, and gradient type 2 (the covariant gradient) is SMCMC_ERR_UNSUPPORTED, whichever of type and mode is set
 * first.  The central point (:391-395, 733-744) stays with the caller, as in pooled mode.  Per-chain state that does not
 * fit in device memory fails Start with SMCMC_ERR_HIP.  Set before smcmc_hmc_start (SMCMC_ERR_LOGIC after it); other
 * modes are SMCMC_ERR_INVALID. */
int smcmc_hmc_set_mode(smcmc_hmc* h, int mode);
int smcmc_hmc_get_mode(const smcmc_hmc* h);
/* chain `chain`'s fAveragePoint [dim], fEstimatedCovariance [dim*dim] and tuning[10] in the layout of
 * smcmc_hmc_get_tuning; any pointer may be NULL.  In SMCMC_MODE_POOLED the shared values. */
int smcmc_hmc_read_chain_tuning(smcmc_hmc* h, int chain, double* average, double* covariance, double* tuning);
/* nsteps x Step(false) of the whole ensemble in SMCMC_MODE_PER_CHAIN (any tuning, any gradient type the mode serves)
 * with a per-step record of one chain in the HOST array records[step * smcmc_hmc_record_stride()]: [0, dim) fAccepted,
 * [dim, 2 dim) fAveragePoint, then the scalars of smcmc_hmc_record_field.  A row is the chain after that step and after
 * the UpdateCovariance / UpdateErrorMatrix that follows it: what smcmc_hmc_read_state, the lanes and
 * smcmc_hmc_read_chain_tuning(h, chain, ...) would return at that moment, i.e. what the branches of TSimpleHMC.H:139-147
 * hold.  POTENTIAL / PROPOSED_POTENTIAL are fAcceptedPotential / fProposedPotential (minus SMCMC_LANE_LOGL /
 * SMCMC_LANE_LOGL_PROPOSED), LEAPFROG is signed as fLeapFrogSteps is, TUNING0 + k is field k of smcmc_hmc_get_tuning.
 * Nothing waits on the host between the steps: a gather kernel after each step's update fills a device row, one copy to
 * the host ends the call.  SMCMC_ERR_UNSUPPORTED outside SMCMC_MODE_PER_CHAIN (the pooled update decides on the host);
 * SMCMC_ERR_INVALID: chain out of range, records NULL, not started. */
typedef enum {
    SMCMC_HMC_REC_POTENTIAL = 0, SMCMC_HMC_REC_PROPOSED_POTENTIAL, SMCMC_HMC_REC_ACCEPTANCE, SMCMC_HMC_REC_LAST_ACCEPT,
    SMCMC_HMC_REC_MEAN_EPSILON, SMCMC_HMC_REC_LEAPFROG, SMCMC_HMC_REC_REVERSAL_LEN, SMCMC_HMC_REC_STEP_COUNT,
    SMCMC_HMC_REC_TUNING0,   /* ... ten fields, the layout of smcmc_hmc_get_tuning */
    SMCMC_HMC_REC_COUNT_ = SMCMC_HMC_REC_TUNING0 + 10
} smcmc_hmc_record_field;
int smcmc_hmc_record_stride(const smcmc_hmc* h);    /* 2 dim + SMCMC_HMC_REC_COUNT_; 0 for NULL */
int smcmc_hmc_step_recorded(smcmc_hmc* h, int nsteps, int chain, double* records);
/* The contract of smcmc_snapshot / smcmc_rollback for a started SMCMC_MODE_PER_CHAIN HMC ensemble: the snapshot holds
 * positions, momenta, both lane tables, the points UpdateCovariance folds, every chain's fAveragePoint, fEXXT, repaired
 * diagonal and tuning scalars, and the step count; rollback returns to it any number of times.  Draws are keyed on
 * (chain, step), so stepping again repeats the same steps.  Settings the engine keeps on the host -- alpha, the
 * gradient type, the gradient matrix -- are not part of the snapshot and stay as they are at a rollback.
 * smcmc_hmc_set_mean_epsilon and smcmc_hmc_set_leapfrog of a started engine are different: they write every chain's
 * fMeanEpsilon / fLeapFrogSteps lanes, and the lanes ARE in the snapshot, so a rollback puts the lanes back to what they
 * were when the snapshot was taken (the engine's host copy, which only the next Start reads, keeps the new value): set
 * them again after the rollback, or, as TSimpleHMC_amd.H does, roll back first and set them afterwards.
 * The snapshot is a second copy of the per-chain state, fEXXT included (dim (dim + 1) / 2 doubles per padded chain):
 * when it does not fit, smcmc_hmc_snapshot is SMCMC_ERR_HIP, keeps nothing and leaves the engine as it was.
 * smcmc_hmc_start discards the snapshot.  Outside the mode SMCMC_ERR_UNSUPPORTED; not started SMCMC_ERR_INVALID; a
 * rollback without a snapshot SMCMC_ERR_LOGIC. */
int smcmc_hmc_snapshot(smcmc_hmc* h);
int smcmc_hmc_rollback(smcmc_hmc* h);

/* ---- variable-at-a-time chains: TSimpleMCMC<L, TProposeVAATStep> ---------
 * N independent chains of sMCMC::TSimpleMCMC<L, sMCMC::TProposeVAATStep> (TProposeVAATStep.H:22-307, the proposal
 * SimpleVAAT.C drives): one coordinate per step from a shuffled queue of the dimensions (:52-78, 177-195), a proposal
 * width per dimension adapted to a 44 % acceptance (:219-255).  Nothing is shared between chains; chain c is the
 * reference chain on the random stream (seed, chain_offset + c).  Every likelihood id of smcmc_likelihood (USER in a
 * library built with one); dim <= 512.  The reference's quirks are kept: Start resets the acceptance window to 100
 * the first time (:211), SetGaussian's sigma is the width of Gaus() unsquared (:69-78), RestoreState / AttachState /
 * SaveState do nothing (:33-36). */
typedef struct smcmc_vaat smcmc_vaat;
int smcmc_vaat_create(int dim, int nchains, int likelihood, uint64_t seed, uint32_t chain_offset, int device,
                      smcmc_vaat** out);
int smcmc_vaat_destroy(smcmc_vaat* h);
const char* smcmc_vaat_last_error(const smcmc_vaat* h);
int smcmc_vaat_set_stream(smcmc_vaat* h, void* hip_stream);
int smcmc_vaat_set_likelihood_params(smcmc_vaat* h, const double* params, int count);
int smcmc_vaat_set_exact_arithmetic(smcmc_vaat* h, int exact);           /* 0: fused multiply-add order; before Start */
int smcmc_vaat_set_uniform(smcmc_vaat* h, int dim, double minimum, double maximum);   /* SetUniform  :101 */
int smcmc_vaat_set_gaussian(smcmc_vaat* h, int dim, double sigma);                    /* SetGaussian :123 */
int smcmc_vaat_set_acceptance_window(smcmc_vaat* h, double a);           /* SetAcceptanceWindow :137 (an int member) */
int smcmc_vaat_get_acceptance_window(const smcmc_vaat* h, double* a);
int smcmc_vaat_set_acceptance_rigidity(smcmc_vaat* h, double r);         /* SetAcceptanceRigidity :148 */
int smcmc_vaat_get_acceptance_rigidity(const smcmc_vaat* h, double* r);
int smcmc_vaat_set_step_rms_window(smcmc_vaat* h, int window);           /* TSimpleMCMC::SetStepRMSWindow */
int smcmc_vaat_start(smcmc_vaat* h, const double* x0, int broadcast);    /* TSimpleMCMC::Start + InitializeState :198 */
int smcmc_vaat_update_proposal(smcmc_vaat* h);                           /* UpdateProposal :177 (SimpleVAAT.C:44) */
int smcmc_vaat_step(smcmc_vaat* h, int nsteps);                          /* nsteps x TSimpleMCMC::Step(false) */
/* as smcmc_step_save: the accepted point [slot][dim][npad] (and logL [slot][npad]) after every stride-th step */
int smcmc_vaat_step_save(smcmc_vaat* h, int nsteps, int stride, double* save_x_device, double* save_logl_device);
int smcmc_vaat_total_steps(const smcmc_vaat* h);
int smcmc_vaat_queue_length(const smcmc_vaat* h);                        /* entries left in fNextIndex */
int smcmc_vaat_nchains_padded(const smcmc_vaat* h);
int smcmc_vaat_read_state(smcmc_vaat* h, double* x, double* logl);       /* GetAccepted, x[dim][nchains] */
/* lanes: SMCMC_LANE_LOGL / LAST_VALUE / STEP_RMS / LOGL_PROPOSED; TRIALS / SUCCESSES / NACCEPT / STEP_RMS_TRIALS /
 * LAST_ACCEPT and SMCMC_VAAT_LANE_LAST_INDEX (fLastIndex) */
#define SMCMC_VAAT_LANE_LAST_INDEX SMCMC_LANE_NEXT_UPDATE
#define SMCMC_VAAT_LANE_PROPOSED_VALUE SMCMC_LANE_LAST_X0   /* f64: fProposed[fLastIndex] of the latest step */
int smcmc_vaat_read_lane_f64(smcmc_vaat* h, int field, double* out);
int smcmc_vaat_read_lane_i32(smcmc_vaat* h, int field, int32_t* out);
/* per-dimension state as [dim][nchains] */
#define SMCMC_VAAT_DIM_SIGMA 0              /* f64 fSigma            :296 */
#define SMCMC_VAAT_DIM_ACCEPTANCE 1         /* f64 fAcceptance       :287 */
#define SMCMC_VAAT_DIM_ACCEPTANCE_TRIALS 2  /* i32 fAcceptanceTrials :290 */
#define SMCMC_VAAT_DIM_QUEUE 3              /* i32 fNextIndex        :266 (slots >= queue length are stale) */
int smcmc_vaat_read_dim_f64(smcmc_vaat* h, int field, double* out);
int smcmc_vaat_read_dim_i32(smcmc_vaat* h, int field, int32_t* out);
int smcmc_vaat_state_device_ptr(smcmc_vaat* h, double** x, double** logl);
/* smcmc_vaat_step(h, nsteps) for every chain, in one launch, with a per-step record of one chain in the HOST array
 * records[step * smcmc_vaat_record_stride()]: the caller's loop around TSimpleMCMC::Step() (SimpleVAAT.C:47-61) without
 * the host in every step.  A step changes ONE coordinate (TProposeVAATStep.H:58-78) and adapts ONE dimension's width
 * (:237-254), so a row is SMCMC_VAAT_REC_COUNT_ scalars whatever the dimension is, and a reader rebuilds the chain from
 * the state at the start of the call plus the rows: x[INDEX] = ACCEPTED_VALUE and nothing else moves; fSigma /
 * fAcceptance / fAcceptanceTrials [ADAPT_INDEX] = ADAPT_* and no other entry changes.  The row after a step holds what
 * the engine would read back after that step:
 *   LOGL, LOGL_PROPOSED, STEP_RMS                  the lanes of the same names (TSimpleMCMC.H:568, 589, 580)
 *   LAST_ACCEPT, TRIALS, SUCCESSES, NACCEPT, STEP_RMS_TRIALS   the integer lanes, as doubles
 *   INDEX                                          fLastIndex, the coordinate this step proposed (:58)
 *   PROPOSED_VALUE                                 fProposed[INDEX] (:62, 77)
 *   ACCEPTED_VALUE                                 fAccepted[INDEX] after the Metropolis test (TSimpleMCMC.H:432-491): the
 *                                                  old value on a rejection
 *   ADAPT_INDEX                                    the dimension whose width UpdateState adapted at the top of this step
 *                                                  (:237-254: the previous step's index), -1 when there was none
 *                                                  (fLastIndex < 0 after Start or the explicit UpdateProposal, :183, 235)
 *   ADAPT_SIGMA, ADAPT_ACCEPTANCE, ADAPT_TRIALS    that dimension's fSigma / fAcceptance / fAcceptanceTrials after the
 *                                                  update, written whether or not the width moved; +0 when ADAPT_INDEX is -1
 *   TOTAL_STEPS, QUEUE_LENGTH                      fTotalSteps (TSimpleMCMC.H:376) and the entries left in fNextIndex
 * In both arithmetic orders, for every likelihood id the library serves and both kernels (dim <= smcmc_max_dim()), any
 * number of chains.  The lane that owns the chain writes its row from inside the step kernel (instantiations of their
 * own: smcmc_vaat_step runs the code it ran before); one copy to the host ends the call.  Calls may be cut anywhere:
 * step_recorded(a) then step_recorded(b) gives the rows of step_recorded(a + b).  SMCMC_ERR_INVALID, with nothing
 * launched and nothing written: NULL handle, not started, records NULL, nsteps < 1, chain outside [0, nchains). */
typedef enum {
    SMCMC_VAAT_REC_LOGL = 0, SMCMC_VAAT_REC_LOGL_PROPOSED, SMCMC_VAAT_REC_STEP_RMS, SMCMC_VAAT_REC_LAST_ACCEPT,
    SMCMC_VAAT_REC_TRIALS, SMCMC_VAAT_REC_SUCCESSES, SMCMC_VAAT_REC_NACCEPT, SMCMC_VAAT_REC_STEP_RMS_TRIALS,
    SMCMC_VAAT_REC_INDEX, SMCMC_VAAT_REC_PROPOSED_VALUE, SMCMC_VAAT_REC_ACCEPTED_VALUE, SMCMC_VAAT_REC_ADAPT_INDEX,
    SMCMC_VAAT_REC_ADAPT_SIGMA, SMCMC_VAAT_REC_ADAPT_ACCEPTANCE, SMCMC_VAAT_REC_ADAPT_TRIALS, SMCMC_VAAT_REC_TOTAL_STEPS,
    SMCMC_VAAT_REC_QUEUE_LENGTH,
    SMCMC_VAAT_REC_COUNT_
} smcmc_vaat_record_field;
int smcmc_vaat_record_stride(const smcmc_vaat* h);    /* SMCMC_VAAT_REC_COUNT_, independent of dim; 0 for NULL */
int smcmc_vaat_step_recorded(smcmc_vaat* h, int nsteps, int chain, double* records);
/* The contract of smcmc_snapshot / smcmc_rollback for a started variable-at-a-time ensemble: the snapshot holds device
 * copies of the whole state -- the points, both lane tables, every chain's fSigma / fAcceptance / fAcceptanceTrials and
 * index queue -- plus the step count, the queue length and the started / initialised flags; rollback returns to it any
 * number of times.  Draws are keyed on (chain, step), so stepping again repeats the same steps.  Settings -- proposal
 * types, acceptance window and rigidity, StepRMS window, likelihood parameters -- are not part of the snapshot and stay
 * as they are at a rollback.  The copies are a second ensemble on the device, freed by smcmc_vaat_destroy: when they do
 * not fit, smcmc_vaat_snapshot is SMCMC_ERR_HIP, keeps nothing and leaves the engine as it was.  Not started
 * SMCMC_ERR_INVALID; a rollback without a snapshot SMCMC_ERR_LOGIC. */
int smcmc_vaat_snapshot(smcmc_vaat* h);
int smcmc_vaat_rollback(smcmc_vaat* h);

/* ---- self test (no engine needed) --------------------------------------- */
/* Runs every function of include/smcmc_detmath.h on the device for n inputs so
 * tests can compare device and host bit for bit.  kind: 0 log, 1 exp,
 * 2 sin(2 pi x), 3 cos(2 pi x), 4 pow_small(x, y), 5 sqrt, 6 x / y, 7 / 8 the two normals of
 * the Box-Muller pair made from the 32-bit words x, y, 9 sqrt_mid, 10 erf, 11 atan.
 * device = -1 evaluates kinds 0, 1, 10 and 11 on the host instead (no GPU needed; other kinds SMCMC_ERR_INVALID):
 * the host side of the comparison, and what tests/event_sample_ref.py builds its deterministic restatement on. */
int smcmc_selftest_detmath(int device, int kind, int n, const double* x, const double* y, double* out);
/* One v_mfma_f64_16x16x4_f64 chain: c[16][16] = sum_k a[16][k] b[k][16] over K
 * (multiple of 4), the accumulation order the pooled moments rely on. */
int smcmc_selftest_mfma(int device, int K, const double* a, const double* b, double* c);
/* The same for v_mfma_f64_4x4x4_4b_f64 as the moment fold uses it: c[4][16] = sum_k a[4][k] b[k][16]. */
int smcmc_selftest_mfma_strip(int device, int K, const double* a, const double* b, double* c);
/* UpdateErrorMatrix's eigenvalue step (TSimpleHMC.H:760-830) on one covariance cov[dim*dim] (dim <= 512) with
 * fEstimatedCovarianceTrace = est_trace: device >= 0 runs SMCMC_MODE_PER_CHAIN's device routine on that device,
 * device < 0 the host routine of the pooled mode.  out[dim*dim + dim + 5]: the covariance after the repair loop
 * (dim*dim), the eigenvalues of its last pass (dim), then max scale, min scale, the number of repair passes,
 * fCurrentCovarianceTrace and fEstimatedOrbitLength. */
int smcmc_selftest_hmc_error_matrix(int device, int dim, double est_trace, const double* cov, double* out);

/* ---- posterior reducer: autocorrelation of a saved trace ----------------------
 * MakeAutocorrelation.C:108-148 defines a(lag) = (E[x_t x_(t-lag)] - mean^2) / var per dimension.
 * This takes its sums on the device from a trace smcmc_step_save wrote
 * (trace_device[slot][dim_stride][nchains_padded]), pooled over slots and chains, about the
 * reference point `centre` ([dim] host; NULL = 0 is the macro's definition, another point changes a(lag)
 * only through the edges of the lagged sums, O(lag / nslots), and conditions E[xx] - mean^2 better):
 *   sum[d]       = sum_{t, c} y            y = x[t][d][c] - centre[d]
 *   lagged[k][d] = sum_{t >= k, c} y_t y_(t-k)     k = 0 .. SMCMC_AUTOCORR_LAGS - 1
 * (host outputs; the number of terms is (nslots - k) * nchains).  Raw sums so that ranks can add
 * theirs.  Fixed summation order: the same bits on every run.  `stream` is a hipStream_t or NULL. */
#define SMCMC_AUTOCORR_LAGS 64
int smcmc_autocorrelation_sums(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                               int nchains_padded, const double* centre, double* sum, double* lagged, void* stream);

/* ---- posterior reducer: autocorrelation of a saved trace on a lag grid ---------
 * MakeAutocorrelation.C looks far back along the chain: it evaluates the lags 1, 1 + lagStep, 1 + 2 lagStep, ... < maxLag
 * with maxLag = min(entries - sqrt(entries), 30000) and lagStep = max(1, int(0.5 maxLag / bins)) (:70-73, 98-99, 117),
 * over the last `trials` entries (:105-108), fills them into `bins` bins (:121-122) and turns every bin into
 * a = (v/e - mean^2) / err^2 (:127-147).  This takes the sums of such a grid on the device; trace layout, `centre`,
 * padding rules and `stream` exactly as smcmc_autocorrelation_sums.  With y = x[t][d][c] - centre[d] and
 * k_i = lag_first + i lag_step:
 *   sum[d]       = sum_{t, c} y_t
 *   sumsq[d]     = sum_{t, c} y_t^2                       (lag 0: the variance's sum, whatever the grid)
 *   lagged[i][d] = sum_{t >= k_i, c} y_t y_(t - k_i)      i = 0 .. nlags - 1
 * Host outputs and raw sums so that ranks can add theirs.  Row i has max(nslots - k_i, 0) * nchains terms; a row with
 * k_i >= nslots is exactly +0.0.  Fixed summation order (smcmc_autocorr_grid.hip states it): the same bits on every
 * run; on a finite trace the bits of a row depend on (k_i, lag_step, trace, centre) only, not on lag_first or nlags
 * (a pass skips the leading products with 0 that another computes, which differ for an Inf or a NaN), so a grid split over
 * several calls gives the same rows; with lag_step = 1 every row with k < SMCMC_AUTOCORR_LAGS and `sum` have the bits
 * smcmc_autocorrelation_sums returns on the same finite trace and centre.
 * The bin of a lag is the fixed-width axis rule stated below for the marginals, 0-based and without the under- and
 * overflow counters: bin = (int)(bins * (lag + 0.5) / maxLag).  A bin no lag falls into is 0/0 = NaN, as in the macro.
 * Deviations from the macro, on purpose:
 *   - its ring buffer holds floats (:63): every value is rounded to single precision before it is multiplied; the
 *     trace here holds doubles and the products are taken in double;
 *   - its TH1F sums are floats (:88-93) and stop counting at 2^24; the sums and counts here are doubles;
 *   - it reads one chain; here the chains of an ensemble are pooled into one sum, so one chain is the macro.
 * SMCMC_ERR_INVALID, with nothing launched and nothing written: the argument errors of smcmc_autocorrelation_sums,
 * lag_first < 0, lag_step < 1, nlags < 1, nlags > SMCMC_AUTOCORR_GRID_MAX_LAGS, lag_first + (nlags - 1) lag_step
 * beyond int, sum, sumsq or lagged NULL.  SMCMC_ERR_NO_DEVICE without a GPU. */
#define SMCMC_AUTOCORR_GRID_MAX_LAGS 512   /* the macro never asks for more than 398 (entries = 420: maxLag = 399, lagStep = 1) */
int smcmc_autocorrelation_grid_sums(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                    int nchains_padded, const double* centre, int lag_first, int lag_step, int nlags,
                                    double* sum, double* sumsq, double* lagged, void* stream);

/* ---- posterior reducer: marginal and pair histograms of a saved trace ----------
 * TestMarginalization.C says WHAT is histogrammed, in three passes over the entries (here: every slot of every live
 * chain of trace_device[slot][dim_stride][nchains_padded], as smcmc_step_save, smcmc_vaat_step_save or
 * smcmc_hmc_copy_positions wrote it; padding lanes and rows >= dim are never read into a result):
 *   :45-63        ranges: lo[d], hi[d] = min / max of dimension d over a subsample of the entries (the loop's
 *                 `entry += 0.001*entries` visits every (1 + (int)(0.001 * entries))-th one); absMin = min(1E+20, lo[d]),
 *                 absMax = max(-1E+20, hi[d]) over all d follow on the host.  Comparisons as std::min / std::max:
 *                 a NaN never replaces a value (a dimension without any comparable value returns lo = +inf, hi = -inf).
 *   :66-76, 97-98 a 1-D histogram of 100 bins over [absMin, absMax) for every dimension;
 *   :78-92, 99-103 for the first min(dim, 10) dimensions and every ordered pair (i, j), (i, i) included, a 50 x 50 histogram,
 *                 x = dimension i, y = dimension j, each over its own range widened by 5 % of its width on both sides.
 * Here the bins, the axes and the list of pair dimensions are the caller's.  The binning is ROOT's fixed-width axis
 * (TAxis::FindBin for equal bins), stated here because ROOT is not available to check it against -- this rule IS the
 * engine's definition and is NOT pinned against ROOT:
 *   bin(x; n, lo, hi) = 0                                    if x < lo          (underflow)
 *                     = n + 1                                if !(x < hi)       (overflow; NaN lands here)
 *                     = 1 + (int)(n * (x - lo) / (hi - lo))  otherwise
 * in IEEE double, un-fused, the division correctly rounded.  A value just below hi whose quotient rounds up to n gets
 * n + 1: the formula's behaviour, kept.  An axis has n + 2 counters, 0 and n + 1 being under- and overflow (ROOT's
 * layout).  Counters are unsigned 64-bit integers: the macro's TH1F holds floats and stops counting at 2^24, which is
 * NOT reproduced.  An axis needs finite ends with lo < hi (SMCMC_ERR_INVALID otherwise; the range pass returns an
 * infinite end when the trace holds one, and the fill then refuses it).
 *   counts1[d][b]        b = bin(x[t][d][c]; n1, lo1[d], hi1[d])                                    d < dim
 *   counts2[p][q][a][b]  a = bin(x[t][pair_dims[p]][c]; n2, lo2[p], hi2[p]), b = the same for q     p, q < npair_dims
 * Host outputs and raw results so that ranks can combine theirs: min / max for ranges, integer addition for counts
 * (exact: the same counts on every run).  n1 = 0 or counts1 = NULL skips the 1-D part, npair_dims = 0 the pair part;
 * one of them must be asked for.  `stream` is a hipStream_t or NULL. */
#define SMCMC_MARGINAL_MAX_BINS1 1000       /* n1: sixteen private copies of the histogram in 64 KB of LDS */
#define SMCMC_MARGINAL_MAX_BINS2 126        /* n2: two tables of 128 x 128 counters in LDS */
#define SMCMC_MARGINAL_MAX_PAIR_DIMS 32     /* npair_dims */
int smcmc_trace_ranges(const double* trace_device, int nslots, int dim, int dim_stride, int nchains, int nchains_padded,
                       int sample_stride, double* lo, double* hi, void* stream);
int smcmc_marginal_histograms(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                              int nchains_padded, int n1, const double* lo1, const double* hi1, uint64_t* counts1,
                              int npair_dims, const int32_t* pair_dims, int n2, const double* lo2, const double* hi2,
                              uint64_t* counts2, void* stream);

/* ---- posterior reducer: mean and covariance of a saved trace -------------------
 * MakeCovariance.C:63-89 adds up, over the entries of the tree, avg[i] += x_i and cov(i, j) += x_i x_j, then takes
 * cov / entries - avg_i avg_j (:84).  This takes the two sums on the device, over every slot of every live chain of
 * trace_device[slot][dim_stride][nchains_padded] (as smcmc_step_save, smcmc_vaat_step_save or smcmc_hmc_copy_positions
 * wrote it; padding lanes and rows >= dim are never read into a result), about the reference point `centre` ([dim]
 * host; NULL = the origin is the macro's definition; the covariance does not depend on it and E[yy] - E[y]E[y] cancels
 * less about a point near the mean): with y = x[t][d][c] - centre[d],
 *   sum[d]      = sum_{t, c} y_d
 *   sumsq[i][j] = sum_{t, c} y_i y_j       dim x dim, row-major, exactly symmetric (the lower triangle, mirrored)
 * Host outputs and raw sums so that ranks can add theirs; the number of terms is nslots * nchains.  The products run
 * on the matrix pipe (one fused multiply-add per term, k over the chains); the summation order is fixed
 * (smcmc_trace_moments.hip states it): the same bits on every run.  Arguments as smcmc_autocorrelation_sums, and
 * dim <= smcmc_max_dim().  `stream` is a hipStream_t or NULL. */
int smcmc_trace_moments(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                        int nchains_padded, const double* centre, double* sum, double* sumsq, void* stream);

/* ---- posterior reducer: split R-hat and multi-chain ESS of a saved trace --------
 * The reducers above pool slots and chains into one sum, which is the reference's single chain.  An ensemble can also be
 * asked whether its chains agree: the split potential scale reduction (Gelman-Rubin in the split form) and the
 * effective sample size built on it (Geyer's truncation; BDA3 section 11.5, Vehtari et al. 2021).  The reference has
 * no counterpart, so this definition IS the engine's.  Over trace_device[slot][dim_stride][nchains_padded] (as
 * smcmc_step_save, smcmc_vaat_step_save or smcmc_hmc_copy_positions wrote it; padding lanes and rows >= dim are never
 * read into a result) and about the reference point `centre` ([dim] host; NULL = the origin):
 *   segments     every live chain c < nchains is cut into S = nsegments >= 1 segments of L = nslots / S slots (integer
 *                division); segment s covers the slots [r + s L, r + (s + 1) L), r = nslots - S L; the r earliest slots
 *                are not read.  S = 2 is split R-hat, S = 1 the plain form.  M = S * nchains segment-chains m = (s, c).
 *   per m        y_t = x[t][d][c] - centre[d];  s1_m[d] = sum_t y_t, slots ascending;  mean_m = s1_m / L (one
 *                division);  z_t = y_t - mean_m (the two subtractions in this order)
 *   sum[d]           = sum_m s1_m[d]
 *   sumsq_of_sums[d] = sum_m s1_m[d]^2
 *   within[k][d]     = sum_m sum_{t = k}^{L - 1} z_t z_(t-k)        k = 0 .. SMCMC_AUTOCORR_LAGS - 1
 *                lags never reach across a segment's first slot; rows k >= L are 0; within[0] is the within-chain sum
 *                of squares.
 * Host outputs and raw sums so that ranks can add theirs (the same L and centre are required).  From them, on the host:
 * W = within[0] / (M (L - 1)), the variance of the segment means (sumsq_of_sums / L^2 - (sum / L)^2 / M) / (M - 1),
 * var+ = (L - 1) / L W + that, R-hat = sqrt(var+ / W), rho_k = 1 - (W - within[k] / (M L)) / var+.
 * chain_sums_device: optional device output [S][dim][nchains_padded] that receives s1 (lanes >= nchains get 0); it is
 * the intermediate of the second pass, so the caller gets per-chain means without another reducer.  NULL: a scratch
 * buffer of the call's own.
 * Fixed summation order (smcmc_convergence.hip states it): the same bits on every run.
 * SMCMC_ERR_INVALID, with nothing launched and nothing written: nsegments < 1, L < 2, dim < 1 or dim > smcmc_max_dim(),
 * dim_stride < dim, nchains < 1, nchains_padded < nchains or not a multiple of 64, trace_device, sum, sumsq_of_sums or
 * within NULL.  SMCMC_ERR_UNSUPPORTED, likewise: nsegments > 65535.  `stream` is a hipStream_t or NULL. */
int smcmc_trace_convergence(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                            int nchains_padded, int nsegments, const double* centre, double* chain_sums_device,
                            double* sum, double* sumsq_of_sums, double* within, void* stream);

/* ---- posterior reducer: the event family's histograms over a saved trace ----------
 * FakeLikelihood::WriteSimulation (example/FakeLikelihood.H:173-179, example2/FakeLikelihood.H:201-207,
 * example3/FakeLikelihood.H:232-239) writes the simulated histograms at ONE point, and every FakeMCMC.C draws them over the
 * data after a burn-in or a cycle.  This is that product for every point of a saved trace: the posterior mean and spread of
 * every histogram bin, the band around the prediction.
 *   likelihood   SMCMC_LIKE_EVENT_SAMPLE, SMCMC_LIKE_EVENT_TEMPLATE or SMCMC_LIKE_EVENT_SHAPE; dim = 9, 9 or 31 is implied
 *   params       that likelihood's flat parameter array [count], under the rules of smcmc_set_likelihood_params
 *   rows         NH * nbins, NH = 3, 3 or 4: the histograms laid end to end in the order of the host evaluators' `hist`
 * Over trace_device[slot][dim_stride][nchains_padded] (as smcmc_step_save wrote it; rows >= dim and lanes >= nchains are
 * never read into a result): for every slot t and live chain c < nchains, h[t][.][c] and logl[t][c] are `hist` and `*logl`
 * of the likelihood's host evaluator (smcmc_event_sample_evaluate, _template_, _shape_) at x[t][0 .. dim)[c], bit for bit,
 * NaN as NaN -- the bin contents for the event sample, the expectation before the clamp for the other two.  With
 * y = h[t][r][c] - centre[r] (`centre`: [rows] host; NULL = the origin):
 *   sum[r]   = sum_{t, c < nchains} y
 *   sumsq[r] = sum_{t, c < nchains} y * y       the product rounded once, then added (un-fused, as everywhere in the family)
 * Host outputs [rows] and raw sums so that ranks can add theirs; the number of terms is nslots * nchains.  A point that
 * makes a class's integral 0 gives NaN histograms on the host and here, and the NaN goes into its rows' sums.
 * hist_device: optional device output [slot][rows][nchains_padded] that receives h itself, lanes >= nchains +0.0: the raw
 * material of bin-to-bin covariances and per-bin quantiles.  logl_device: optional device output [slot][nchains_padded],
 * the layout of smcmc_step_save's save_logl, likewise.
 * Fixed summation order (smcmc_event_predictive.hip states it): the same bits on every run, a function of (params, trace,
 * centre, nslots, nchains) alone -- not of whether the optional outputs are asked for, nor of what the padding lanes hold.
 * SMCMC_ERR_INVALID, with nothing launched and nothing written: another likelihood; a parameter array that breaks a rule
 * (the text through smcmc_event_sample_last_error, as the evaluators give it); nslots < 1, dim_stride < dim, nchains < 1,
 * nchains_padded < nchains or not a multiple of 64, trace_device NULL; sum or sumsq NULL.  SMCMC_ERR_NO_DEVICE without a
 * GPU, checked after all of these.  `stream` is a hipStream_t or NULL. */
int smcmc_event_predictive_sums(int likelihood, const double* params, int count, const double* trace_device, int nslots,
                                int dim_stride, int nchains, int nchains_padded, const double* centre, double* hist_device,
                                double* logl_device, double* sum, double* sumsq, void* stream);

/* ---- posterior reducer: exact order statistics of a saved trace (quantiles, credible intervals) ----
 * The median and the 68 % / 95 % credible interval of a parameter, or the quantile band of a predicted bin, are order
 * statistics of a row of the trace: selected values, not sums, so the result is the bits of an entry and the same on every
 * run.  The reference has no counterpart; this definition IS the engine's, not numpy's or ROOT's.
 *   the order   with b the 64 bits of a double, key(x) = b ^ (b >> 63 ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000), and
 *               every NaN, of either sign, gets key = 0xFFFFFFFFFFFFFFFF.  Unsigned comparison of keys is the total order
 *               -inf < ... < -0 < +0 < ... < +inf < NaN.  value(key) is the inverse, the quiet NaN 0x7FF8000000000000 for
 *               the all-ones key.  One copy for host and device: include/smcmc_order_key.h; the two host functions below
 *               are that copy.
 *   a row       the N = nslots * nchains entries x[t][d][c], c < nchains, of trace_device[slot][dim_stride][nchains_padded]
 *               (as smcmc_step_save, smcmc_vaat_step_save or smcmc_hmc_copy_positions wrote it, or the hist_device of
 *               smcmc_event_predictive_sums with dim = dim_stride = rows).  Padding lanes and rows >= dim are never read
 *               into a result.  dim is not bounded by the largest dimension the kernels step: it is bounded by the grid,
 *               dim <= SMCMC_ORDER_MAX_DIM.
 * The selection is a radix selection from the most significant byte down: SMCMC_ORDER_PASSES passes of
 * SMCMC_ORDER_DIGIT_BITS bits.
 *
 * The pass primitive (what ranks combine): pass p in 0 .. 7, prefixes[d][i] (host, [dim][nprefix]) the top 8p bits of a
 * key, right-aligned; ignored at p = 0, where it may be NULL.  counts[d][i][g] (host, [dim][nprefix][256]) receives the
 * number of entries of row d with  key >> (64 - 8p) == prefixes[d][i]  and  (key >> (56 - 8p)) & 255 == g  (at p = 0 the
 * first condition is empty).  A prefix with bits above its 8p is matched by no entry.  Counts are integers: ranks add
 * theirs exactly, and every run gives the same numbers.
 *
 * The reducer: ranks[r] (host, [nranks]) are zero-based, each < N; repeats and any order are allowed.
 *   values[d][r]   the entry of row d with exactly ranks[r] entries before it in key order, as value(key): the bits of an
 *                  entry of the trace, a NaN as the canonical one
 *   below[d][r]    optional: the number of entries of row d with a smaller key than that entry's
 *   equal[d][r]    optional: the number with the same key (>= 1).  below <= ranks[r] < below + equal; a Metropolis trace
 *                  repeats a value at every rejected step, so ties are the normal case
 * all host, [dim][nranks].  Eight passes of the primitive's kernel run on `stream`; between passes a small kernel picks each
 * (row, rank)'s digit from the 256 counts and carries the residual rank; the host synchronises once, at the end.
 *
 * SMCMC_ERR_INVALID, with nothing launched and nothing written: trace_device, ranks, values (the reducer), counts or, at
 * p > 0, prefixes (the primitive) NULL; nranks < 1 or > SMCMC_ORDER_MAX_RANKS; a rank >= N; nslots < 1; dim < 1 or
 * > SMCMC_ORDER_MAX_DIM; dim_stride < dim; nchains < 1; nchains_padded < nchains or not a multiple of 64; pass outside
 * 0 .. 7; nprefix outside 1 .. SMCMC_ORDER_MAX_RANKS.  SMCMC_ERR_NO_DEVICE without a GPU, checked after all of these.
 * `stream` is a hipStream_t or NULL. */
#define SMCMC_ORDER_DIGIT_BITS 8
#define SMCMC_ORDER_PASSES 8
#define SMCMC_ORDER_MAX_RANKS 32
#define SMCMC_ORDER_MAX_DIM 65535           /* rows: the grid's y extent */
uint64_t smcmc_order_key(double x);
double smcmc_order_value(uint64_t key);
int smcmc_order_chunk_entries(void);        /* entries of a row one workgroup counts (more only where a launch would exceed 2 048 workgroups) */
int smcmc_trace_digit_counts(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                             int nchains_padded, int pass, int nprefix, const uint64_t* prefixes, uint64_t* counts,
                             void* stream);
int smcmc_trace_order_statistics(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                 int nchains_padded, int nranks, const uint64_t* ranks, double* values, uint64_t* below,
                                 uint64_t* equal, void* stream);

/* ---- posterior reducer: the posterior-predictive check (replicated data and p-values) ----
 * The band of smcmc_event_predictive_sums is around the EXPECTATION of a bin; the data scatter about it with Poisson noise.
 * Whether the data fit the model is asked of replicated data: for every posterior point draw y_rep[r] ~ Poisson(mu[r]) from
 * that point's expectation, compare the likelihood's own discrepancy on the replicate with the one on the observed data,
 * and report the tail fractions (Gelman, Meng and Stern 1996).  The reference has no counterpart -- every FakeMCMC.C draws
 * dataStack over the prediction and leaves the question to the eye -- so this definition IS the engine's.
 *   the variate  include/smcmc_poisson.h states it line by line: mu = max(expectation, 0.001), the clamp of the bin term; one
 *                Philox block per variate at (seed, global chain, step = global slot | row << 28 | replica << 44) on
 *                SMCMC_STREAM_REPLICA; a 52-bit uniform; inversion of the cumulative distribution from 0 (mu < 16) or
 *                outwards from the mode (mu >= 16).  A function of its inputs alone, the same bits on host and device.  It
 *                is INVALID, and nothing is drawn, for an expectation that is NaN or infinite or mu > SMCMC_POISSON_MAX_MEAN.
 *                smcmc_poisson_draw is that variate on the host (no GPU needed): `chain` and `slot` are the global ones;
 *                *valid = 0 and *y = NaN when invalid.  SMCMC_ERR_INVALID, nothing written: y or valid NULL, slot >= 2^28,
 *                row >= 2^16, replica >= 2^16.
 *   input        hist_device[slot][rows][nchains_padded]: what smcmc_event_predictive_sums leaves in its hist_device, or any
 *                buffer of Poisson means in that layout; lanes >= nchains are never read into a result.  data[rows]: host,
 *                finite and >= 0.  Group g of ngroups is the rows [g rows / ngroups, (g + 1) rows / ngroups): for the event
 *                family one group per histogram.
 *   a point      (t, c < nchains) is VALID when the variate is at every one of its rows.  For a valid point
 *                  y[r]     = the variate at (seed, chain_offset + c, slot_offset + t, r, replica) and mu[r]
 *                  T_obs[g] = sum_r smcmc_es_bin_term(data[r], mu[r]),  T_rep[g] = sum_r smcmc_es_bin_term(y[r], mu[r])
 *                over the group's rows ascending from +0.0, un-fused (include/smcmc_event_sample.h); entry g = ngroups holds
 *                the same two sums over all rows, as running sums of their own.  For SMCMC_LIKE_EVENT_SAMPLE the total
 *                T_obs is the likelihood's logl, bit for bit.
 *   results      host, all INTEGERS -- ranks, windows of slots and replicas add theirs exactly; the same numbers on every
 *                run and on every grid:
 *                  below[r], equal[r]       the valid points with y[r] < data[r], with y[r] == data[r]           [rows]
 *                  stat_counts[g][3]        the valid points with T_rep < T_obs, with T_rep == T_obs, and the number
 *                                           compared                                                  [ngroups + 1][3]
 *                  *invalid                 the invalid points; they enter nothing else
 *   rep_device   optional device output [slot][rows][nchains_padded]: y as doubles, NaN in every row of an invalid point,
 *                +0.0 in lanes >= nchains -- the layout smcmc_trace_order_statistics takes: its quantiles are the band the
 *                DATA are expected to lie in.
 *   stat_device  optional device output [slot][2 (ngroups + 1)][nchains_padded]: row 2 g is T_obs, row 2 g + 1 is T_rep,
 *                invalid points and padding likewise.  The reducers over a trace take it as it is.
 * The p-value of group g is (stat_counts[g][0] + stat_counts[g][1]) / stat_counts[g][2].
 * SMCMC_ERR_INVALID, with nothing launched and nothing written: hist_device, data, below, equal, stat_counts or invalid
 * NULL; nslots < 1, rows outside 1 .. SMCMC_PREDICTIVE_CHECK_MAX_ROWS, nchains < 1, nchains_padded < nchains or not a
 * multiple of 64; ngroups outside 1 .. SMCMC_PREDICTIVE_CHECK_MAX_GROUPS or not dividing rows; a data[r] that is negative
 * or not finite; slot_offset + nslots > 2^28 or replica >= 2^16 (the text through smcmc_event_sample_last_error).
 * SMCMC_ERR_NO_DEVICE without a GPU, checked after all of these.  `stream` is a hipStream_t or NULL. */
#define SMCMC_POISSON_MAX_MEAN 1048576.0
#define SMCMC_PREDICTIVE_CHECK_MAX_ROWS 4096    /* two 64-bit counters per row in 64 KB of LDS */
#define SMCMC_PREDICTIVE_CHECK_MAX_GROUPS 8
int smcmc_poisson_draw(uint64_t seed, uint32_t chain, uint32_t slot, uint32_t row, uint32_t replica, double expectation,
                       double* y, int* valid);
int smcmc_predictive_check(const double* hist_device, int nslots, int rows, int nchains, int nchains_padded,
                           const double* data, int ngroups, uint64_t seed, uint32_t chain_offset, uint32_t slot_offset,
                           uint32_t replica, double* rep_device, double* stat_device, uint64_t* below, uint64_t* equal,
                           uint64_t* stat_counts, uint64_t* invalid, void* stream);

/* ---- the Gaussian stand-in chain of a mean and a covariance ---------------------
 * CholeskyChain.C:18-66: covariance = U^T U with U upper triangular (:39-46; here the row-ordered routine the adaptive
 * proposal uses, a pivot that is not positive and finite is SMCMC_ERR_RUNTIME and nothing is launched or written, where
 * the macro exits), then every entry is
 *   accepted = mean;  for i ascending: r_i = Gaus(0, 1), accepted[j] += r_i * U(i, j) for all j       (:53-60)
 * with an un-fused multiply and add.  Every (slot, chain < nchains) of trace_device[slot][dim_stride][nchains_padded]
 * gets one entry; rows >= dim and lanes >= nchains are not written.  The normals of an entry are laid out as a
 * chain-step's: Philox block b of counter (b, chain_offset + chain, slot) on stream SMCMC_STREAM_CHOLESKY gives the
 * normals 4b .. 4b + 3, words (0, 1) and (2, 3) one pair of the engine's normal transform each
 * (include/smcmc_detmath.h).  The draws are keyed on the global chain number, so a fill with a chain_offset is a slice
 * of the whole fill.  mean[dim] and covariance[dim*dim] (its upper triangle is read) are host arrays; `decomposition`
 * is an optional [dim*dim] host output, U row-major.  dim <= smcmc_max_dim(), nchains_padded a multiple of 64.  The
 * result is a trace the reducers above take as it is.  `stream` is a hipStream_t or NULL. */
int smcmc_cholesky_chain(const double* mean, const double* covariance, int dim, int nslots, int nchains,
                         int nchains_padded, int dim_stride, uint64_t seed, uint32_t chain_offset,
                         double* trace_device, double* decomposition, void* stream);

#ifdef __cplusplus
}
#endif
#endif
