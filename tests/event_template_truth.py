"""SMCMC_LIKE_EVENT_TEMPLATE in high precision: the definition of include/smcmc.h, for the tests that pin the host
evaluation to it.

The per-event part -- the corrected mass, the scaled separation, the cuts, the split and the bin -- is
SMCMC_LIKE_EVENT_SAMPLE's and comes from EventSampleTruth (tests/event_sample_truth.py), with the decision gap it
reports.  Steps 1 to 6 of the definition are restated here in real arithmetic (mpmath at event_sample_truth.PREC bits),
sharing no floating-point order with tests/event_template_ref.py or include/smcmc_event_sample.h:

  example2/SystematicCorrection.H:76-115   weight = c / t or (1 - c) / (1 - t), c = atan(tan(pi (t - 1/2)) + q) / pi + 1/2,
                                           (t, q) = (trueFakes, p7) for a signal and (trueEfficiency, p8) for a background
                                           event: no exp(p0 / 10), no exposure
  example2/FakeLikelihood.H:232-264        S[h][b], B[h][b]: the weights of the Type 0 / Type > 0 events of a bin, added
  :266-277                                 IS, IB: everything in the class's three histograms (dropped events are in none);
                                           ws = p0 / IS, wb = p1 / IB
  :280-288                                 mc = ws S + wb B
  :64-89                                   logL = sum of data - m + (data > 0 ? data ln(m / data) : 0), m = max(mc, 0.001)
  :91-115                                  if p0 < 0: logL -= 10 + |logL|; the same for p1; logL -= (p6 / 5)^2 / 2,
                                           p7^2 / 2, p8^2 / 2

A mutation of the definition is a subclass that replaces one of the small methods below.
"""
import importlib.util
import os
from collections import namedtuple

import mpmath
from mpmath import mpf

_spec = importlib.util.spec_from_file_location("smcmc_event_sample_truth",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_sample_truth.py"))
sample_truth = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sample_truth)

PREC = sample_truth.PREC
exact = sample_truth.exact

Result = namedtuple("Result", "logl bins S B IS IB ws wb mc terms where gap mass event log_args")
# bins: the bin sum before the penalties; S, B, mc, terms: [3 nbins]; where, gap, mass: EventSampleTruth's;
# event: what evaluate() got from EventSampleTruth (its exp and log arguments among it)


class EventTemplateTruth:
    FLOOR = exact(0.001)
    TEN = exact(10.0)
    FIVE = exact(5.0)
    HALF = exact(0.5)

    def __init__(self, params, per_event=None):
        """per_event: an EventSampleTruth of the same params to share (a mutation of steps 1 to 6 leaves it alone)"""
        self.per_event = per_event or sample_truth.EventSampleTruth(params)
        E = self.per_event
        self.nbins, self.nevents = E.nbins, E.nevents
        self.background = [e[4] for e in E.events]
        self.tagged = [e[5] for e in E.events]

    # ---- the pieces a mutation replaces ----
    def weights(self, p):
        """[background][tagged]"""
        E = self.per_event
        cf = E.corrected_probability(E.tan_fakes, p[7])
        ce = E.corrected_probability(E.tan_efficiency, p[8])
        tf, te = E.true_fakes, E.true_efficiency
        return [[(1 - cf) / (1 - tf), cf / tf], [(1 - ce) / (1 - te), ce / te]]

    def integral(self, hist, dropped):
        """hist: the class's 3 nbins bins; dropped: the weights of its events that a cut or the axis dropped"""
        return mpmath.fsum(hist)

    def norms(self, p, IS, IB):
        return p[0] / IS, p[1] / IB

    def sign_penalty(self, logl):
        return logl - (10 + abs(logl))

    def gaussian_penalties(self, p):
        return [self.HALF * (p[6] / self.FIVE) ** 2, self.HALF * p[7] ** 2, self.HALF * p[8] ** 2]

    # ---- the definition ----
    def evaluate(self, point, event=None):
        """event: per_event.evaluate(point), if the caller has it already"""
        with mpmath.workprec(PREC):
            return self._evaluate([exact(v) for v in point], event or self.per_event.evaluate(point))

    def _evaluate(self, p, ev):
        nbins = self.nbins
        w = self.weights(p)
        S, B = [mpf(0)] * (3 * nbins), [mpf(0)] * (3 * nbins)
        dropped = [[], []]
        for k, background, tagged in zip(ev.where, self.background, self.tagged):
            if k < 0:
                dropped[background].append(w[background][tagged])
            elif background:
                B[k] += w[1][tagged]
            else:
                S[k] += w[0][tagged]
        IS, IB = self.integral(S, dropped[0]), self.integral(B, dropped[1])
        ws, wb = self.norms(p, IS, IB)
        mc = [ws * s + wb * b for s, b in zip(S, B)]
        terms, log_args = [], []
        data = [d for h in range(3) for d in self.per_event.data_of(h)]
        for d, m in zip(data, mc):
            m = max(m, self.FLOOR)
            v = d - m
            if d > 0:
                v += d * mpmath.log(m / d)
                log_args.append(m / d)
            terms.append(v)
        bins = mpmath.fsum(terms)
        logl = bins
        if p[0] < 0:
            logl = self.sign_penalty(logl)
        if p[1] < 0:
            logl = self.sign_penalty(logl)
        for t in self.gaussian_penalties(p):
            logl -= t
        return Result(logl, bins, S, B, IS, IB, ws, wb, mc, terms, ev.where, ev.gap, ev.mass, ev, log_args)
