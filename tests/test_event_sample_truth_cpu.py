"""SMCMC_LIKE_EVENT_SAMPLE on the host (smcmc_event_sample_evaluate) against the definition in high precision
(tests/event_sample_truth.py), without a GPU.  The device kernels are held to the host bit for bit elsewhere
(tests/test_gpu_event_sample*.py), so this is what says that the value they all agree on is the right one.

u = 2^-53.  E_exp, E_log, E_erf, E_atan: the largest error of smcmc_exp, smcmc_log, smcmc_erf, smcmc_atan against their
TRUE values, in ulp of the true value (measured against mpmath by test_deterministic_functions_against_their_true_values
below, not assumed); an ulp is at most 2 u of the value, so a function's relative error is at most 2 E u.  Everything
below is first order in u; the bounds are multiplied by 1 + 2^-20, which covers the second-order terms as long as a bound
stays below 2^-21 relative (they are below 1e-12).

THE FIXTURES.  A bound on a bin's content only makes sense while host and truth put the same events into the bin.  Every
evaluation used here has a decision gap (event_sample_truth.py) of at least GAP = 1e-9, asserted, while the host's
corrected mass is within 1e-13 of the true one (below, and asserted for a few events per case) and its bin quotient
nbins (m - xmin) / (xmax - xmin) carries three more roundings: no event may change bin or cut, and the test asserts that
the host's bins are the truth's.  A case that falls under the gap gets another key, never a smaller gap.

A WEIGHT (SystematicCorrection.H:81-117), w = exp(p_k / 10) r X.
  exp(p_k / 10)      the quotient is rounded (u relative, |p_k / 10| u in the exponent, so in the value) and
                     the function adds 2 E_exp u:                                     (|p_k| / 10 + 2 E_exp) u
  q = atan(s) / pi   s = tan + p is rounded once (u), which moves atan(s) by at most u relative because
                     |s atan'(s) / atan(s)| <= 1; the function adds 2 E_atan u, the division u:
                                                                                       (2 + 2 E_atan) u relative
  c = q + 1/2        the addition cancels when q is near -1/2 (trueFakes = 0.05: q = -0.45): the absolute error of q,
                     |q| (2 + 2 E_atan) u, stays and is divided by c; the addition rounds:
                                                                         (|q| / c) (2 + 2 E_atan) u + u
  1 - c              again the absolute error of c stays, divided by 1 - c; the subtraction rounds:
                                                          ((|q| (2 + 2 E_atan) + c) / (1 - c)) u + u
  r                  c / t: one division.  (1 - c) / (1 - t): 1 - t is rounded, and one division.
  the two products   2 u
so  c_w = |p_k| / 10 + 2 E_exp + 3 + (|q| / c) (2 + 2 E_atan) + 1                    for MuDk > 0
    c_w = |p_k| / 10 + 2 E_exp + 4 + (|q| (2 + 2 E_atan) + c) / (1 - c) + 1          otherwise,
with q and c the true values at the point.

A BIN'S CONTENT is the sum of its n_k events' weights, all positive, by n_k - 1 roundings (the first addition, to +0,
is exact).  The sum of positive terms keeps relative errors: |host - truth| <= (n_k - 1 + c_w) u truth, c_w the largest
over the classes of the bin's events.  An empty bin is +0 on both sides.

logL (FakeLikelihood.H:47-81) = sum of term_k = d - mc + d ln(mc / d), mc = max(content, 0.001), d the data.  Let
dmc_k be the bound on the content above, or 0 when content (1 + bound) < 0.001 (both sides clamp to the same double; the
clamp never increases a difference).  Then
  d - mc             dmc_k, and the subtraction rounds: u |d - mc|
  mc / d             dmc_k / mc relative, and u; the logarithm turns a relative error of its argument into the same
                     absolute error, times d: d (dmc_k / mc + u) -- the conditioning of the logarithm
  ln                 2 E_log u |ln(mc / d)|, the product with d one more u: d |ln(mc / d)| (2 E_log + 1) u
  the addition       u |term_k|
and the 3 nbins terms are added up by 3 nbins - 1 roundings (the first, to +0, is exact): gamma_m sum |term_k| with
m = 3 nbins - 1.  bound(logL) = sum_k (the five lines above) + gamma_m sum_k |term_k|.

THE CORRECTED MASS (SystematicCorrection.H:50-79), for the events whose host mass the test recovers by bisection on
xmax.  With a = |ln T|, N = ln(T + S) - ln T, D = ln M - ln T, z = D / N, k = 0.3 erf(p4 / 10), g = exp(z k),
w = exp(p3 / 10), absolute errors in units of u:
  e_A = 2 E_log a                                    ln T
  e_N = 2 E_log (a + |ln(T + S)|) + 1 + N            T + S rounded (u relative, u in the logarithm), the subtraction
  e_D = 2 E_log (a + |ln M|) + |D|
  e_z = |z| + e_D / N + |z| e_N / N                  the division, and both operands
  e_k = |k| (2 + 2 E_erf)                            p4 / 10 rounded: |x erf'(x) / erf(x)| <= 1; erf; the product
  e_q = |k| e_z + |z| e_k + |z k|                    the exponent z k
  r_g = e_q + 2 E_exp,  r_w = |p3| / 10 + 2 E_exp    relative errors of g and w
  e_1 = 2 e_A + e_D g + |D| g (r_g + 2) + |ln T + D g|          (ln T + D g) - ln T      :72 and the difference of :73
  e_2 = e_1 w + |D| g w (r_w + 1)                                                    the product of :73
  e_3 = e_A + e_2 + |lm2|,  lm2 = ln T + D g w                                       the sum of :73
  e_4 = e_3 + |p2| / 10 + |lm2 + p2 / 10|                                            :64 and :74
and the mass, exp of that, is off by (e_4 + 2 E_exp) u relative.  For |ln| <= 7 this is a few 1e-14.

THE MUTATIONS.  test_mutations_are_caught applies each of them to a copy of the truth and requires that at least one case
leaves the bound: the bounds above are tight enough to tell 0.5 from 0.5 (1 + 1e-13).
"""
import importlib.util
import itertools
import math
import os

import mpmath
import numpy as np
import pytest
from mpmath import mpf

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("smcmc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref, cases, truth = _load("event_sample_ref"), _load("event_sample_cases"), _load("event_sample_truth")

U = mpf(2) ** -53
SECOND_ORDER = 1 + mpf(2) ** -20
GAP = 1e-9
# ulp of the true value; test_deterministic_functions_against_their_true_values holds each to its measurement
E_EXP, E_LOG, E_ERF, E_ATAN = 1.0, 1.0, 1.5, 1.0
PROBED_POINTS = (1, cases.NPOINTS - 1)      # a generic point, and the one with the skew beyond the switch of smcmc_erf


# ---- the bounds of the docstring ----------------------------------------------------------------------------------
def weight_constants(T, p):
    """c_w[background][tagged]"""
    out = []
    for k, tangent, shift in ((0, T.tan_fakes, p[7]), (1, T.tan_efficiency, p[8])):
        c = T.corrected_probability(tangent, shift)
        q = abs(c - T.HALF)
        common = abs(p[k]) / 10 + 2 * E_EXP
        out.append([common + 4 + (q * (2 + 2 * E_ATAN) + c) / (1 - c) + 1, common + 3 + (q / c) * (2 + 2 * E_ATAN) + 1])
    return out


def content_bounds(T, p, r, classes):
    """relative bound per bin, from the truth's `where` and the events' classes"""
    cw = weight_constants(T, p)
    n, worst = [0] * (3 * T.nbins), [mpf(0)] * (3 * T.nbins)
    for (background, tagged), k in zip(classes, r.where):
        if k >= 0:
            n[k] += 1
            worst[k] = max(worst[k], cw[background][tagged])
    return [(n[k] - 1 + worst[k]) * U * SECOND_ORDER if n[k] else mpf(0) for k in range(3 * T.nbins)]


def logl_bound(T, r, rel):
    total, size = mpf(0), mpf(0)
    data = [d for h in range(3) for d in T.data_of(h)]
    for k, (d, content, term) in enumerate(zip(data, r.hist, r.terms)):
        mc = max(content, T.FLOOR)
        dmc = rel[k] * content if content * (1 + rel[k]) >= T.FLOOR else mpf(0)
        e = dmc + U * abs(d - mc)
        if d > 0:
            e += d * (dmc / mc + U) + d * abs(mpmath.log(mc / d)) * (2 * E_LOG + 1) * U
        total += e + U * abs(term)
        size += abs(term)
    m = 3 * T.nbins - 1
    return (total + m * U / (1 - m * U) * size) * SECOND_ORDER


def mass_bound(T, p, i):
    """relative"""
    n, d, z = T.events[i][:3]
    true_mass, with_sigma, mass = T.sample_log_args[3 * i:3 * i + 3]
    a, N = abs(n), mpmath.log(with_sigma) - n
    L, X = 2 * E_LOG, 2 * E_EXP
    e_a = L * a
    e_n = L * (a + abs(mpmath.log(with_sigma))) + 1 + N
    e_d = L * (a + abs(mpmath.log(mass))) + abs(d)
    e_z = abs(z) + e_d / N + abs(z) * e_n / N
    k = T.SKEW_LIMIT * mpmath.erf(p[4] / 10)
    e_k = abs(k) * (2 + 2 * E_ERF)
    e_q = abs(k) * e_z + abs(z) * e_k + abs(z * k)
    g, w = mpmath.exp(z * k), mpmath.exp(p[3] / 10)
    r_g, r_w = e_q + X, abs(p[3]) / 10 + X
    e_1 = 2 * e_a + e_d * g + abs(d) * g * (r_g + 2) + abs(n + d * g)
    e_2 = e_1 * w + abs(d) * g * w * (r_w + 1)
    lm2 = n + d * g * w
    e_3 = e_a + e_2 + abs(lm2)
    e_4 = e_3 + abs(p[2]) / 10 + abs(lm2 + p[2] / 10)
    return (e_4 + X) * U * SECOND_ORDER


# ---- the host's side ----------------------------------------------------------------------------------------------
def host_mass(smcmc, params, i, point):
    """The host's corrected mass of event i (below 500), to the bit: alone in a sample of one bin on [0, x) the event
    is kept exactly when mass < x, so the largest double x that drops it is the mass."""
    prm = cases.one_event(params, i)
    nbins = int(prm[1])
    prm = np.concatenate([prm[:8], np.ones(3), prm[8 + 3 * nbins:]])
    prm[1], prm[2] = 1.0, 0.0

    def kept(x):
        prm[3] = x
        return bool(np.any(smcmc.event_sample_evaluate(prm, point, histograms=True)[1]))

    lo, hi = 2.0 ** -20, 500.0
    assert kept(hi) and not kept(lo)
    while np.nextafter(lo, np.inf) < hi:
        mid = lo + (hi - lo) / 2
        lo, hi = (lo, mid) if kept(mid) else (mid, hi)
    return lo


class Case:
    """one sample: its points, the host's values at them, what is needed to judge a truth against them"""
    def __init__(self, name, oracle, smcmc):
        self.name = name
        self.params = cases.sample(ref, oracle, name)
        self.points = cases.points(ref, oracle, name)
        ev = ref.split(self.params)[-1]
        self.classes = [(int(e[1] > 0), int(e[3] > 0)) for e in ev]
        self.host = [smcmc.event_sample_evaluate(self.params, p, histograms=True) for p in self.points]
        self.truth = truth.EventSampleTruth(self.params)
        self.results = [self.truth.evaluate(p) for p in self.points]
        # a few events whose host mass is recovered: spread over the sample, inside (1, 499) at the probed points
        self.probes = []
        for j in PROBED_POINTS:
            inside = [i for i, m in enumerate(self.results[j].mass) if 1 < m < 499]
            for i in inside[::max(1, len(inside) // 3)][:3]:
                self.probes.append((j, i, host_mass(smcmc, self.params, i, self.points[j])))

    def ratios(self, T, j, r=None):
        """(worst error / bound over the bins, the same for logL) of the host at point j, judged by the truth T"""
        with mpmath.workprec(truth.PREC):
            r = r or T.evaluate(self.points[j])
            p = [mpf(float(v)) for v in self.points[j]]
            logl, hist = self.host[j]
            rel = content_bounds(T, p, r, self.classes)
            worst = 0.0
            for got, want, bound in zip(hist.ravel(), r.hist, rel):
                err = abs(mpf(float(got)) - want)
                if err > 0:
                    worst = max(worst, float(err / (bound * want)) if bound * want > 0 else math.inf)
            return worst, float(abs(mpf(logl) - r.logl) / logl_bound(T, r, rel))

    def mass_ratios(self, T):
        out = []
        with mpmath.workprec(truth.PREC):
            for j, i, got in self.probes:
                p = [mpf(float(v)) for v in self.points[j]]
                want = T.evaluate(self.points[j]).mass[i] if T is not self.truth else self.results[j].mass[i]
                out.append(float(abs(mpf(got) - want) / want / mass_bound(T, p, i)))
        return out


@pytest.fixture(scope="module")
def world(oracle, smcmc):
    return {name: Case(name, oracle, smcmc) for name in cases.CASES}


@pytest.fixture(params=list(cases.CASES))
def case(request, world):
    return world[request.param]


# ---- the tests ----------------------------------------------------------------------------------------------------
def test_no_decision_within_the_gap_and_the_host_bins_are_the_truths(case, smcmc):
    smallest = min(float(r.gap) for r in case.results)
    print("%s: smallest decision gap over %d points %.3e" % (case.name, len(case.points), smallest))
    assert smallest >= GAP
    for p, r in zip(case.points, case.results):
        assert cases.host_where(smcmc, case.params, p) == [max(k, -1) for k in r.where]
    r0 = case.results[0]                        # the origin: the separation that is exactly the cut is not Close
    assert r0.sep[0] == case.truth.cut and not 0 <= r0.where[0] < case.truth.nbins


def test_host_definition_within_the_derived_bound(case):
    worst = [case.ratios(case.truth, j, r) for j, r in enumerate(case.results)]
    bins, logl = max(w[0] for w in worst), max(w[1] for w in worst)
    print("%s: worst error / bound  bin contents %.3f  logL %.3f" % (case.name, bins, logl))
    assert bins <= 1.0 and logl <= 1.0


def test_host_corrected_mass_within_the_derived_bound(case):
    assert case.probes
    worst = max(case.mass_ratios(case.truth))
    print("%s: corrected mass of %d events, worst error / bound %.3f" % (case.name, len(case.probes), worst))
    assert worst <= 1.0
    with mpmath.workprec(truth.PREC):
        for j, i, got in case.probes:
            assert mass_bound(case.truth, [mpf(float(v)) for v in case.points[j]], i) <= 1e-13


def _ulp_errors(got, true_values):
    """|got - true| in units of the spacing of doubles at the true value"""
    out = []
    for g, t in zip(got, true_values):
        nearest = float(t)
        if math.isinf(nearest) or (nearest == 0.0 and g == 0.0):
            continue
        out.append(float(abs(mpf(float(g)) - t) / mpf(float(np.spacing(abs(nearest))))))
    return np.array(out)


def test_deterministic_functions_against_their_true_values(world, smcmc):
    """E_exp, E_log at the arguments the likelihood forms in these cases (the doubles nearest the true arguments),
    E_erf, E_atan on the grids of tests/event_sample_ref.py: against mpmath, which rounds nothing at this precision."""
    log_args = np.unique([float(a) for c in world.values() for r in c.results for a in r.log_args])
    exp_args = np.unique([float(a) for c in world.values() for r in c.results for a in r.exp_args])
    measured = {}
    with mpmath.workprec(128):
        for name, kind, fn, x in (("E_exp", 1, mpmath.exp, exp_args), ("E_log", 0, mpmath.log, log_args),
                                  ("E_erf", 10, mpmath.erf, ref.erf_grid()), ("E_atan", 11, mpmath.atan, ref.atan_grid())):
            x = np.ascontiguousarray(x, dtype=np.float64)
            err = _ulp_errors(smcmc.selftest_detmath(kind, x, device=-1), [fn(mpf(float(v))) for v in x])
            measured[name] = float(err.max())
            print("%s: %d arguments, largest error %.4f ulp of the true value" % (name, x.size, err.max()))
    for name, constant in (("E_exp", E_EXP), ("E_log", E_LOG), ("E_erf", E_ERF), ("E_atan", E_ATAN)):
        assert measured[name] <= constant <= math.ceil(2.0 * measured[name]) / 2.0, name


def _mutations():
    T = truth.EventSampleTruth
    out = {}
    classes = [(0, 0), (0, 1), (1, 0), (1, 1)]
    for a, b in itertools.combinations(classes, 2):
        def weights(self, p, a=a, b=b):
            w = T.weights(self, p)
            w[a[0]][a[1]], w[b[0]][b[1]] = w[b[0]][b[1]], w[a[0]][a[1]]
            return w
        out["weight classes %r and %r exchanged" % (a, b)] = {"weights": weights}

    def swapped(self, params):
        T.__init__(self, params)
        self.true_fakes, self.true_efficiency = self.true_efficiency, self.true_fakes
        self.tan_fakes, self.tan_efficiency = self.tan_efficiency, self.tan_fakes
    out["trueFakes and trueEfficiency exchanged"] = {"__init__": swapped}
    out["0.3 (1 + 1e-12)"] = {"SKEW_LIMIT": T.SKEW_LIMIT * (1 + mpf(10) ** -12)}
    out["separation <= cut is Close"] = {"is_close": lambda self, sep: sep <= self.cut}
    out["bin index + 1"] = {"bin_of": lambda self, mass: min(T.bin_of(self, mass) + 1, self.nbins - 1)}
    out["bin index + 1 without the clamp"] = {"bin_of": lambda self, mass: T.bin_of(self, mass) + 1}
    out["clamp at 0.0011"] = {"FLOOR": mpf(0.0011)}

    def no_exposure(self, params):
        T.__init__(self, params)
        self.exposure = mpf(1)
    out["exposure dropped"] = {"__init__": no_exposure}
    out["0.5 (1 + 1e-13)"] = {"HALF": T.HALF * (1 + mpf(10) ** -13)}
    out["Close's data taken from Separated's row"] = {"data_of": lambda self, h: self.data[1 if h == 0 else h]}
    out["the last event left out"] = {"sample": lambda self: self.events[:-1]}
    return out


MUTATIONS = _mutations()


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutations_are_caught(world, name):
    """the first case and point at which the host leaves the mutated truth's bound"""
    with mpmath.workprec(truth.PREC):       # (the mutated constants above are made of exact parts)
        Mutant = type("Mutant", (truth.EventSampleTruth,), MUTATIONS[name])
    for case in world.values():
        T = Mutant(case.params)
        found = None
        for j in range(len(case.points)):
            bins, logl = case.ratios(T, j)
            if bins > 1.0 or logl > 1.0:
                found = "point %d: bin contents %.3g, logL %.3g x bound" % (j, bins, logl)
                break
        if found is None:
            worst = max(case.mass_ratios(T))
            if worst > 1.0:
                found = "corrected mass %.3g x bound" % worst
        if found:
            print("%s: caught by %s, %s" % (name, case.name, found))
            return
    pytest.fail("no case catches the mutation: " + name)
