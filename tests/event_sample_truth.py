"""SMCMC_LIKE_EVENT_SAMPLE in high precision: the definition, for the tests that pin the host evaluation to it.

Written from the reference's text, in real arithmetic (mpmath at PREC = 256 bits), sharing no code and no
floating-point order with tests/event_sample_ref.py, include/smcmc_event_sample.h, the oracle or the product:

  example/SystematicCorrection.H:35-48    separation' = Separation exp(param[k] / 10), k by Type
  example/SystematicCorrection.H:50-79    with n = ln TrueMass, d = ln(Mass / TrueMass), z = d / ln(1 + Sigma / TrueMass):
                                          ln mass' = n + d exp(0.3 erf(p4 / 10) z + p3 / 10) + p2 / 10
                                          (:72-74 applied one after the other are this one expression: the skew and the
                                          width both multiply the distance d from the nominal log mass, the scale shifts it)
  example/SystematicCorrection.H:81-117   weight = exp(p0 / 10 or p1 / 10) r X, r one of c / t, (1 - c) / (1 - t) with
                                          c = atan(tan(pi (t - 1/2)) + q) / pi + 1/2, (t, q) = (trueFakes, p7) for a signal
                                          event and (trueEfficiency, p8) for a background event, X the exposure ratio
  example/FakeLikelihood.H:188-216        the cuts (mass' > 500, mass' < 0, separation' < 0 drop the event), DecayTag if
                                          MuDk > 0, else Close if separation' < cut, else Separated
  include/smcmc.h, "the bin rule"         for xmin <= mass' < xmax the bin is floor(nbins (mass' - xmin) / (xmax - xmin)),
                                          at most nbins - 1; anything else is dropped
  example/FakeLikelihood.H:47-81          logL = sum over Close, Separated, DecayTag and their bins of
                                          data - mc + (data > 0 ? data ln(mc / data) : 0), mc = max(content, 0.001)

Conventions.  Every input (the parameter array, the point) enters as the exact value of its double.  The literals of the
reference text (0.3, 0.5, 10.0, 500.0, 0.001, M_PI) are the exact values of the doubles a compiler makes of them, as in
tests/truth.py.  tan(pi (t - 1/2)) is a constant of the sample which include/smcmc.h says the host takes from libm when
it packs the parameters: it enters here as the exact value of the double math.tan(math.pi * (t - 0.5)), not as the real
tangent -- with the real one the truth would be that of a different sample constant, off by libm's rounding times the
conditioning of 1/2 + atan / pi.  Nothing else is rounded before a comparison is made.

evaluate() also returns the decision gap of the evaluation: over all events, the smallest relative distance
|v - t| / max(|v|, |t|) of the corrected mass to 500, xmin, xmax and every bin edge xmin + k (xmax - xmin) / nbins, and
of the scaled separation to the cut.  A value equal to its threshold in real arithmetic does not count (the fixture's
separation 100 exp(0) at the origin): there the comparison above decides, and no rounding of a faithful evaluation can
change it unless the evaluation rounds exp(0).  Thresholds at zero (mass' < 0, separation' < 0, xmin = 0) are at relative
distance one from every positive value and are left out.
Of the bin edges the two on either side of the mass are looked at: every other edge is further away.

A mutation of the definition, for the tests that show their bound bites, is a subclass that replaces one of the
constants or one of the small methods below.
"""
import math
from collections import namedtuple

import mpmath
from mpmath import mpf

PREC = 256

Result = namedtuple("Result", "logl hist where gap mass sep weights terms log_args exp_args")
# logl, hist[3 nbins], mass[nevents], sep[nevents], weights[type > 0][MuDk > 0], terms[3 nbins]: mpf
# where[nevents]: the flat bin (Close 0 .. nbins - 1, Separated, DecayTag) or -1 mass > 500, -2 mass < 0,
#                 -3 separation < 0, -4 outside the axis
# log_args, exp_args: the real arguments of every logarithm and exponential the definition takes (for the tests that
#                 measure the product's log and exp where the likelihood uses them)


def exact(x):
    return mpf(float(x))


class EventSampleTruth:
    SKEW_LIMIT = exact(0.3)         # SystematicCorrection.H:68
    HALF = exact(0.5)               # :96, :108
    TEN = exact(10.0)
    MASS_CEILING = exact(500.0)     # FakeLikelihood.H:203
    FLOOR = exact(0.001)            # :56
    PI = exact(math.pi)             # M_PI

    def __init__(self, params):
        prm = [float(v) for v in params]
        self.nevents, self.nbins = int(prm[0]), int(prm[1])
        assert len(prm) == 8 + 3 * self.nbins + 6 * self.nevents
        with mpmath.workprec(PREC):
            self.xmin, self.xmax, self.exposure, self.cut = (exact(v) for v in prm[2:6])
            self.true_fakes, self.true_efficiency = exact(prm[6]), exact(prm[7])
            self.tan_fakes = exact(math.tan(math.pi * (prm[6] - 0.5)))
            self.tan_efficiency = exact(math.tan(math.pi * (prm[7] - 0.5)))
            self.data = [[exact(v) for v in prm[8 + h * self.nbins:8 + (h + 1) * self.nbins]] for h in range(3)]
            self.events, self.sample_log_args = [], []
            for i in range(self.nevents):
                mass, typ, sep, mudk, true_mass, sigma = (exact(v) for v in prm[8 + 3 * self.nbins + 6 * i:][:6])
                n = mpmath.log(true_mass)
                d = mpmath.log(mass / true_mass)
                z = d / mpmath.log(1 + sigma / true_mass)
                self.events.append((n, d, z, sep, typ > 0, mudk > 0))
                self.sample_log_args += [true_mass, true_mass + sigma, mass]

    # ---- the pieces a mutation replaces ----
    def corrected_probability(self, tangent, shift):
        return mpmath.atan(tangent + shift) / self.PI + self.HALF

    def weights(self, p):
        """[background][tagged]"""
        cf = self.corrected_probability(self.tan_fakes, p[7])
        ce = self.corrected_probability(self.tan_efficiency, p[8])
        tf, te = self.true_fakes, self.true_efficiency
        ws, wb = mpmath.exp(p[0] / self.TEN), mpmath.exp(p[1] / self.TEN)
        return [[ws * (1 - cf) / (1 - tf) * self.exposure, ws * cf / tf * self.exposure],
                [wb * (1 - ce) / (1 - te) * self.exposure, wb * ce / te * self.exposure]]

    def is_close(self, sep):
        return sep < self.cut

    def bin_of(self, mass):
        b = int(mpmath.floor(self.nbins * (mass - self.xmin) / (self.xmax - self.xmin)))
        return min(b, self.nbins - 1)

    def data_of(self, h):
        return self.data[h]

    def sample(self):
        return self.events

    # ---- the definition ----
    def evaluate(self, point):
        with mpmath.workprec(PREC):
            return self._evaluate([exact(v) for v in point])

    def _evaluate(self, p):
        nbins = self.nbins
        skew = self.SKEW_LIMIT * mpmath.erf(p[4] / self.TEN)
        width, shift = p[3] / self.TEN, p[2] / self.TEN
        sep_scale = [mpmath.exp(p[5] / self.TEN), mpmath.exp(p[6] / self.TEN)]
        weight = self.weights(p)
        exp_args = [p[k] / self.TEN for k in (0, 1, 3, 5, 6)]
        width_of_bin = (self.xmax - self.xmin) / nbins
        ends = [self.MASS_CEILING, self.xmin, self.xmax]
        hist = [mpf(0)] * (3 * nbins)
        where, masses, seps, gap = [], [], [], mpf(1)

        def distance(v, t):
            return abs(v - t) / max(abs(v), abs(t))

        for n, d, z, sep0, background, tagged in self.sample():
            log_mass = n + d * mpmath.exp(skew * z + width) + shift
            mass = mpmath.exp(log_mass)
            sep = sep0 * sep_scale[1 if background else 0]
            exp_args += [skew * z, log_mass]
            masses.append(mass)
            seps.append(sep)
            k = min(max(int(mpmath.floor((mass - self.xmin) / width_of_bin)), 0), nbins - 1)    # the nearest edges
            for t in ends + [self.xmin + k * width_of_bin, self.xmin + (k + 1) * width_of_bin]:
                if mass != t and t != 0:
                    gap = min(gap, distance(mass, t))
            if sep != self.cut and self.cut != 0:
                gap = min(gap, distance(sep, self.cut))
            if mass > self.MASS_CEILING:
                where.append(-1)
            elif mass < 0:
                where.append(-2)
            elif sep < 0:
                where.append(-3)
            elif not (self.xmin <= mass < self.xmax):
                where.append(-4)
            else:
                h = 2 if tagged else 0 if self.is_close(sep) else 1
                b = self.bin_of(mass)
                if 0 <= b < nbins:                  # (only a mutated bin rule leaves the axis here)
                    hist[h * nbins + b] += weight[background][tagged]
                    where.append(h * nbins + b)
                else:
                    where.append(-4)

        terms, log_args = [], []
        for h in range(3):
            data = self.data_of(h)
            for b in range(nbins):
                mc = max(hist[h * nbins + b], self.FLOOR)
                v = data[b] - mc
                if data[b] > 0:
                    v += data[b] * mpmath.log(mc / data[b])
                    log_args.append(mc / data[b])
                terms.append(v)
        return Result(mpmath.fsum(terms), hist, where, gap, masses, seps, weight, terms,
                      self.sample_log_args + log_args, exp_args)
