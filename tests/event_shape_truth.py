"""SMCMC_LIKE_EVENT_SHAPE in high precision: the definition of include/smcmc.h, for the tests that pin the host
evaluation to it.

The corrected mass and the scaled separation of an event are SMCMC_LIKE_EVENT_SAMPLE's expressions with example3's
parameter indices; they come from EventSampleTruth (tests/event_sample_truth.py), which is handed the events and a
nine-parameter point in example's order made from the 31 (`systematics`).  Everything else is restated here in real
arithmetic (mpmath at event_sample_truth.PREC bits), sharing no floating-point order with tests/event_shape_ref.py or
include/smcmc_event_shape.h:

  example3/SystematicCorrection.H:78-124   weight = r exp(shape(Mass)), r = c / t or (1 - c) / (1 - t),
                                           c = atan(tan(pi (t - 1/2)) + q / 10) / pi + 1/2, (t, q) = (trueFakes, p4) for a
                                           signal and (trueEfficiency, p5) for a background event; Mass the uncorrected mass
  :136-149                                 yB[i] = p[9 + i] / 10; yS[0] = yS[12] = 0, yS[i + 1] = p[20 + i] / 10
  TFakeGP.H:79-81, TH1::Interpolate        centres low + (i + 1/2) (high - low) / n; y[0] at or below the first, y[n - 1]
                                           at or above the last; else the line through the two centres around x
  example3/FakeLikelihood.H:265-300        the cuts; DecayTag if MuDk > 0, else VeryClose if separation' < cutVeryClose,
                                           else Close if separation' < cutClose, else Separated
  :303-316                                 IS, IB: everything in the class's four histograms; ws = p0 / IS, wb = p1 / IB
  :319-331                                 mc = ws S + wb B
  :68-102                                  logL = sum of data - m + (data > 0 ? data ln(m / data) : 0), m = max(mc, 0.001)
  :104-134                                 if p0 < 0: logL -= 10 + |logL|; the same for p1; logL -= (p3 / 5)^2 / 2, p4^2 / 2,
                                           p5^2 / 2; logL -= yB' KinvB yB; logL -= yS' KinvS yS
The inverted kernels enter as the exact values of the doubles the library made (its `parts`); how good they are as
inverses is a test of its own.

evaluate() returns the decision gap of the evaluation: EventSampleTruth's (the corrected mass against 500, xmin, xmax
and the bin edges around it, the scaled separation against cutClose), and with it the scaled separation against
cutVeryClose and the uncorrected mass against the two centres around it and the first and the last centre of its
class's shape, each as |v - t| / max(|v|, |t|).

A mutation of the definition is a subclass that replaces one of the small methods below.
"""
import importlib.util
import os
from collections import namedtuple

import mpmath
import numpy as np
from mpmath import mpf

_spec = importlib.util.spec_from_file_location("smcmc_event_sample_truth",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_sample_truth.py"))
sample_truth = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sample_truth)

PREC = sample_truth.PREC
exact = sample_truth.exact
HEAD, NB, NS = 12, 11, 13

Result = namedtuple("Result", "logl bins S B IS IB ws wb penB penS mc terms where gap event shape located log_args exp_args")
# bins: the bin sum before the penalties; S, B, mc, terms: [4 nbins]; where[nevents]: the flat bin (VeryClose, Close,
# Separated, DecayTag) or negative; shape[nevents]: the shape's value of every event; located[nevents]: (k, clamped);
# event: EventSampleTruth's result (masses, separations)


def gp_penalty(y, kinv):
    """TFakeGP.H:137-145 in real arithmetic"""
    n = len(y)
    return mpmath.fsum(y[i] * y[j] * kinv[i][j] for i in range(n) for j in range(n))


class EventShapeTruth:
    FLOOR = exact(0.001)
    TEN = exact(10.0)
    FIVE = exact(5.0)
    HALF = exact(0.5)

    def __init__(self, params, kinv_b, kinv_s):
        prm = [float(v) for v in params]
        self.nevents, self.nbins = int(prm[0]), int(prm[1])
        nb = self.nbins
        assert len(prm) == HEAD + 4 * nb + 290 + 6 * self.nevents
        events = prm[HEAD + 4 * nb + 290:]
        # the per-event part: the events under LIKE_EVENT_SAMPLE's header (its data are not looked at)
        self.per_event = sample_truth.EventSampleTruth(prm[:4] + [1.0, prm[5]] + prm[6:8] + [1.0] * (3 * nb) + events)
        E = self.per_event
        with mpmath.workprec(PREC):
            self.cut_very_close, self.cut_close = exact(prm[4]), exact(prm[5])
            self.ranges = [(exact(prm[10]), exact(prm[11]), NS), (exact(prm[8]), exact(prm[9]), NB)]     # [background]
            self.data = [exact(v) for v in prm[HEAD:HEAD + 4 * nb]]
            self.kernel = [[[exact(v) for v in row] for row in np.asarray(prm[HEAD + 4 * nb + 121:HEAD + 4 * nb + 290]).reshape(NS, NS)],
                           [[exact(v) for v in row] for row in np.asarray(prm[HEAD + 4 * nb:HEAD + 4 * nb + 121]).reshape(NB, NB)]]
            self.kinv = [[[exact(v) for v in row] for row in np.asarray(kinv_s)], [[exact(v) for v in row] for row in np.asarray(kinv_b)]]
            self.raw_mass = [exact(events[6 * i]) for i in range(self.nevents)]
        self.background = [e[4] for e in E.events]
        self.tagged = [e[5] for e in E.events]

    # ---- the pieces a mutation replaces ----
    def systematics(self, p):
        """the 31 parameters as a point of LIKE_EVENT_SAMPLE (mass scale, width, skew, the two separation scales in its
        slots 2 to 6; its weights are not used)"""
        return [0.0, 0.0, p[6], p[7], p[8], p[2], p[3], 0.0, 0.0]

    def tag_shifts(self, p):
        """what is added to the two tangents"""
        return p[4] / self.TEN, p[5] / self.TEN

    def control_values(self, p):
        """[background]: the signal's 13, the background's 11"""
        return [[mpf(0)] + [p[20 + i] / self.TEN for i in range(11)] + [mpf(0)], [p[9 + i] / self.TEN for i in range(NB)]]

    def centres(self, background):
        low, high, n = self.ranges[background]
        return [low + (i + self.HALF) * (high - low) / n for i in range(n)]

    def segment(self, x, c, low, high):
        """the control value the line through x starts at (x strictly between the first and the last centre)"""
        n = len(c)
        b = min(int(mpmath.floor(n * (x - low) / (high - low))), n - 1)
        return b - 1 if x <= c[b] else b

    def shape_argument(self, raw_mass, corrected_mass):
        return raw_mass

    def histogram_of(self, sep, tagged):
        return 3 if tagged else 0 if sep < self.cut_very_close else 1 if sep < self.cut_close else 2

    def integral(self, hist):
        return mpmath.fsum(hist)

    def penalty(self, y, background):
        return gp_penalty(y, self.kinv[background])

    def apply_shape_penalty(self, logl, pen):
        return logl - pen

    def gaussian_penalties(self, p):
        return [self.HALF * (p[3] / self.FIVE) ** 2, self.HALF * p[4] ** 2, self.HALF * p[5] ** 2]

    # ---- the definition ----
    def shape(self, x, y, background):
        """-> (value, (k, clamped), gap)"""
        low, high, n = self.ranges[background]
        c = self.centres(background)

        def distance(v, t):
            return abs(v - t) / max(abs(v), abs(t))

        gap = min(distance(x, c[0]), distance(x, c[n - 1]))
        if x <= c[0]:
            return y[0], (0, True), gap
        if x >= c[n - 1]:
            return y[n - 1], (n - 1, True), gap
        k = self.segment(x, c, low, high)
        near = min(max(int(mpmath.floor((x - c[0]) / (c[1] - c[0]))), 0), n - 2)       # the centres around x
        gap = min(gap, distance(x, c[near]), distance(x, c[near + 1]))
        return y[k] + (x - c[k]) * (y[k + 1] - y[k]) / (c[k + 1] - c[k]), (k, False), gap

    def evaluate(self, point):
        with mpmath.workprec(PREC):
            p = [exact(v) for v in point]
            return self._evaluate(p, self.per_event.evaluate([float(v) for v in self.systematics([float(v) for v in point])]))

    def _evaluate(self, p, ev):
        E = self.per_event
        nbins, rows = self.nbins, 4 * self.nbins
        qf, qe = self.tag_shifts(p)
        cf, ce = E.corrected_probability(E.tan_fakes, qf), E.corrected_probability(E.tan_efficiency, qe)
        tf, te = E.true_fakes, E.true_efficiency
        w = [[(1 - cf) / (1 - tf), cf / tf], [(1 - ce) / (1 - te), ce / te]]
        y = self.control_values(p)
        S, B = [mpf(0)] * rows, [mpf(0)] * rows
        where, shapes, located, exp_args = [], [], [], []
        gap = ev.gap
        for i in range(self.nevents):
            background, tagged = self.background[i], self.tagged[i]
            mass, sep = ev.mass[i], ev.sep[i]
            v, loc, g = self.shape(self.shape_argument(self.raw_mass[i], mass), y[background], background)
            shapes.append(v)
            located.append(loc)
            exp_args.append(v)
            gap = min(gap, g)
            if sep != self.cut_very_close and self.cut_very_close != 0:
                gap = min(gap, abs(sep - self.cut_very_close) / max(abs(sep), abs(self.cut_very_close)))
            k = ev.where[i]                     # EventSampleTruth's: negative codes, or its own three histograms' bin
            if k >= 0:
                k = self.histogram_of(sep, tagged) * nbins + k % nbins
                weight = w[background][tagged] * mpmath.exp(v)
                if background:
                    B[k] += weight
                else:
                    S[k] += weight
            where.append(k)
        IS, IB = self.integral(S), self.integral(B)
        ws, wb = p[0] / IS, p[1] / IB
        mc = [ws * s + wb * b for s, b in zip(S, B)]
        terms, log_args = [], []
        for d, m in zip(self.data, mc):
            m = max(m, self.FLOOR)
            v = d - m
            if d > 0:
                v += d * mpmath.log(m / d)
                log_args.append(m / d)
            terms.append(v)
        bins = mpmath.fsum(terms)
        logl = bins
        if p[0] < 0:
            logl = logl - (10 + abs(logl))
        if p[1] < 0:
            logl = logl - (10 + abs(logl))
        for t in self.gaussian_penalties(p):
            logl -= t
        pen_b, pen_s = self.penalty(y[1], 1), self.penalty(y[0], 0)
        logl = self.apply_shape_penalty(logl, pen_b)
        logl = self.apply_shape_penalty(logl, pen_s)
        return Result(logl, bins, S, B, IS, IB, ws, wb, pen_b, pen_s, mc, terms, where, gap, ev, shapes, located, log_args, exp_args)
