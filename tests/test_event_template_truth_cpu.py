"""SMCMC_LIKE_EVENT_TEMPLATE on the host (smcmc_event_template_evaluate) against the definition in high precision
(tests/event_template_truth.py), without a GPU.  The device kernels are held to the host bit for bit elsewhere
(tests/test_gpu_event_template*.py), so this is what says that the value they all agree on is the right one.

The bound is derived the way tests/test_event_sample_truth_cpu.py derives its own, from which the notation comes:
u = 2^-53; E_log, E_atan the largest errors of smcmc_log and smcmc_atan in ulp of the true value (that file measures
E_atan on its grid; E_log is measured below at the arguments this likelihood forms); everything first order in u and
multiplied by 1 + 2^-20 for the second-order terms.

THE FIXTURES.  Every evaluation used here has a decision gap (event_sample_truth.py) of at least GAP = 1e-9, and at
least 1000 times the derived error bound of the corrected mass of every one of its events (mass_bound of
test_event_sample_truth_cpu.py; the bin quotient and the scaled separation carry a handful of roundings more): no event
may change bin, cut or class of histogram between host and truth.  Both are asserted with the truth alone
(test_fixtures_decide_nothing_within_the_gap); a case under the gap would get another key, never a smaller gap.

A WEIGHT (example2/SystematicCorrection.H:76-115) is that file's r: its c_w without the exponential (|p_k| / 10 +
2 E_exp) and without the two products (2), q and c the true values at the point:
    c_w = (|q| / c) (2 + 2 E_atan) + 2                       for MuDk > 0       (c = q + 1/2 rounds, one division)
    c_w = (|q| (2 + 2 E_atan) + c) / (1 - c) + 3             otherwise          (1 - c, 1 - t round, one division)

A BIN'S CONTENT of S or B, n_k events of positive weights: |host - truth| <= r_k truth, r_k = (n_k - 1 + c_w) u, c_w the
largest over the bin's events (that file's per-bin content bound).

AN INTEGRAL (step 2) adds the class's 3 nbins positive contents by at most 3 nbins + 2 additions (the three sums from +0
and the two that join them; those to +0 are exact and counted all the same): a sum of positive terms keeps relative
errors, so r_I = max_k r_k + gamma_m, m = 3 nbins + 2, gamma_m = m u / (1 - m u).  The normalisation is one division of
an exact count: r_w = r_I + u.

THE EXPECTATION (step 3) mc = (0.0 + ws S) + wb B: two products (u each) and one addition (0.0 + x is exact), with
operands of either sign, so the bound is absolute:
    dmc = |ws S| (r_ws + r_S + u) + |wb B| (r_wb + r_B + u) + u |mc|.

A BIN TERM is that file's, with m = max(mc, 0.001), dm = dmc, or 0 when mc + dmc < 0.001 (both sides clamp to the same
double; the clamp never increases a difference):
    dm + u |d - m| + (d > 0 ? d (dm / m + u) + d |ln(m / d)| (2 E_log + 1) u : 0) + u |term|
and the 3 nbins terms are added by 3 nbins - 1 roundings: e_bins = sum of the above + gamma_(3 nbins - 1) sum |term|.

THE PENALTIES (step 5), L the value before and e its bound:
    L' = L - (10 + |L|)     |L| carries e, 10 + |L| rounds, L - (..) carries e again and rounds:
                            e' = 2 e + u (10 + |L|) + u |L'|                                           (each of the two)
    L' = L - (0.5 v) v      v = p / 5 or p / 1 rounds (u, twice in the product), 0.5 v is exact, the product rounds,
                            the subtraction rounds:  e' = e + 3 u t + u |L'|,  t = v^2 / 2             (each of the three)

THE MUTATIONS.  test_mutations_are_caught applies each of them to a copy of the truth and requires that the host leaves
the bound at some case and point.  (exp(p0 / 10) left in the weights cancels in ws S: it is the contents of S, IS and ws
that leave their bounds, which is why every stage is held to its own.)
"""
import importlib.util
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


tref, truth, sample_test = _load("event_template_ref"), _load("event_template_truth"), _load("test_event_sample_truth_cpu")

U = sample_test.U
SECOND_ORDER = sample_test.SECOND_ORDER
GAP = sample_test.GAP
E_LOG, E_ATAN = sample_test.E_LOG, sample_test.E_ATAN
NPOINTS = 12
CASES = {"197ev_50bins": (60, 137, 50, 101), "64ev_5bins": (30, 34, 5, 102), "65ev_97bins": (25, 40, 97, 107)}


def gamma(m):
    return m * U / (1 - m * U)


# ---- the bounds of the docstring ----------------------------------------------------------------------------------
def weight_constants(T, p):
    """c_w[background][tagged]"""
    E = T.per_event
    out = []
    for tangent, shift in ((E.tan_fakes, p[7]), (E.tan_efficiency, p[8])):
        c = E.corrected_probability(tangent, shift)
        q = abs(c - T.HALF)
        out.append([(q * (2 + 2 * E_ATAN) + c) / (1 - c) + 3, (q / c) * (2 + 2 * E_ATAN) + 2])
    return out


def bounds(T, p, r):
    """{"S", "B": relative per bin, "IS", "IB", "ws", "wb": relative, "mc": absolute per bin, "logl": absolute}"""
    rows = 3 * T.nbins
    cw = weight_constants(T, p)
    n = [[0] * rows, [0] * rows]
    worst = [[mpf(0)] * rows, [mpf(0)] * rows]
    for k, background, tagged in zip(r.where, T.background, T.tagged):
        if k >= 0:
            n[background][k] += 1
            worst[background][k] = max(worst[background][k], cw[background][tagged])
    rel = [[(n[c][k] - 1 + worst[c][k]) * U if n[c][k] else mpf(0) for k in range(rows)] for c in range(2)]
    r_i = [max(rel[c]) + gamma(rows + 2) for c in range(2)]
    r_w = [v + U for v in r_i]
    dmc = [abs(r.ws * r.S[k]) * (r_w[0] + rel[0][k] + U) + abs(r.wb * r.B[k]) * (r_w[1] + rel[1][k] + U) + U * abs(r.mc[k])
           for k in range(rows)]
    data = [d for h in range(3) for d in T.per_event.data_of(h)]
    total, size = mpf(0), mpf(0)
    for d, mc, dm, term in zip(data, r.mc, dmc, r.terms):
        m = max(mc, T.FLOOR)
        if mc + dm < T.FLOOR:
            dm = mpf(0)
        e = dm + U * abs(d - m)
        if d > 0:
            e += d * (dm / m + U) + d * abs(mpmath.log(m / d)) * (2 * E_LOG + 1) * U
        total += e + U * abs(term)
        size += abs(term)
    e = total + gamma(rows - 1) * size
    value = r.bins
    for k in (0, 1):
        if p[k] < 0:
            after = value - (10 + abs(value))
            e = 2 * e + U * (10 + abs(value)) + U * abs(after)
            value = after
    for t in (T.HALF * (p[6] / T.FIVE) ** 2, T.HALF * p[7] ** 2, T.HALF * p[8] ** 2):
        value = value - t
        e = e + 3 * U * t + U * abs(value)
    s = SECOND_ORDER
    return {"S": [v * s for v in rel[0]], "B": [v * s for v in rel[1]], "IS": r_i[0] * s, "IB": r_i[1] * s,
            "ws": r_w[0] * s, "wb": r_w[1] * s, "mc": [v * s for v in dmc], "logl": e * s}


def _ratio(got, want, bound):
    err = abs(mpf(float(got)) - want)
    if err == 0:
        return 0.0
    return float(err / bound) if bound > 0 else math.inf


class Case:
    """one sample: its points, the host's values at them, the per-event truth shared by the mutants"""
    def __init__(self, name, oracle, smcmc):
        nsig, nbkg, nbins, key = CASES[name]
        self.name = name
        self.params = tref.make_sample(oracle, nsig, nbkg, nbins, key)
        self.points = tref.points(oracle, NPOINTS, key + 1000, self.params)
        self.host = [smcmc.event_template_evaluate(self.params, p, histograms=True, parts=True) for p in self.points]
        self.truth = truth.EventTemplateTruth(self.params)
        self.events = [self.truth.per_event.evaluate(p) for p in self.points]
        self.results = [self.truth.evaluate(p, ev) for p, ev in zip(self.points, self.events)]

    def ratios(self, T, j, r=None):
        """{stage: worst error / bound} of the host at point j, judged by the truth T"""
        with mpmath.workprec(truth.PREC):
            r = r or T.evaluate(self.points[j], self.events[j])
            p = [mpf(float(v)) for v in self.points[j]]
            b = bounds(T, p, r)
            logl, hist, parts = self.host[j]
            out = {}
            for key, want in (("S", r.S), ("B", r.B)):
                out[key] = max(_ratio(g, w, bd * w) for g, w, bd in zip(parts[key].ravel(), want, b[key]))
            for key, want in (("IS", r.IS), ("IB", r.IB), ("ws", r.ws), ("wb", r.wb)):
                out[key] = _ratio(parts[key], want, b[key] * abs(want))
            out["mc"] = max(_ratio(g, w, bd) for g, w, bd in zip(hist.ravel(), r.mc, b["mc"]))
            out["logl"] = _ratio(logl, r.logl, b["logl"])
            return out


@pytest.fixture(scope="module")
def world(oracle, smcmc):
    return {name: Case(name, oracle, smcmc) for name in CASES}


@pytest.fixture(params=list(CASES))
def case(request, world):
    return world[request.param]


# ---- the tests ----------------------------------------------------------------------------------------------------
def test_fixtures_decide_nothing_within_the_gap(case):
    """with the truth alone: every chosen point's decision gap is at least GAP and far above the corrected mass's bound"""
    E = case.truth.per_event
    worst_mass = 0.0
    with mpmath.workprec(truth.PREC):
        for point, ev in zip(case.points, case.events):
            p = [mpf(float(v)) for v in point]
            bound = max(float(sample_test.mass_bound(E, p, i)) for i in range(E.nevents))
            worst_mass = max(worst_mass, bound)
            assert float(ev.gap) >= GAP and float(ev.gap) >= 1000.0 * bound
    smallest = min(float(ev.gap) for ev in case.events)
    print("%s: smallest decision gap over %d points %.3e, largest bound of a corrected mass %.3e"
          % (case.name, len(case.points), smallest, worst_mass))
    # what the mutations need: a dropped event in each class would be best, one in the background is there by construction;
    # a negative count of either class; points off the origin
    assert all(any(k < 0 and b for k, b in zip(ev.where, case.truth.background)) for ev in case.events)
    assert any(p[0] < 0 for p in case.points) and any(p[1] < 0 for p in case.points)
    assert all(math.isfinite(h[0]) for h in case.host)


def test_host_bins_are_the_truths(case):
    for (logl, hist, parts), r in zip(case.host, case.results):
        for key, want in (("S", r.S), ("B", r.B)):
            assert list(np.flatnonzero(parts[key].ravel())) == [k for k, v in enumerate(want) if v != 0]


def test_host_definition_within_the_derived_bound(case):
    worst = {}
    for j, r in enumerate(case.results):
        for key, v in case.ratios(case.truth, j, r).items():
            worst[key] = max(worst.get(key, 0.0), v)
    print("%s: worst error / bound  %s" % (case.name, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
    with mpmath.workprec(truth.PREC):      # the bound is no licence: a few 1e-13 of the size of the terms
        for j, r in enumerate(case.results):
            b = bounds(case.truth, [mpf(float(v)) for v in case.points[j]], r)
            assert b["logl"] <= 1e-12 * (10 + mpmath.fsum(abs(t) for t in r.terms))


def test_log_at_this_likelihoods_arguments(world, smcmc):
    """E_log where steps 1 to 6 take a logarithm: mc / data"""
    args = np.unique([float(a) for c in world.values() for r in c.results for a in r.log_args])
    with mpmath.workprec(128):
        err = sample_test._ulp_errors(smcmc.selftest_detmath(0, args, device=-1), [mpmath.log(mpf(float(v))) for v in args])
    print("smcmc_log at %d arguments mc / data: largest error %.4f ulp of the true value" % (args.size, err.max()))
    assert err.max() <= E_LOG


def _mutations():
    T = truth.EventTemplateTruth
    out = {}
    out["ws taken from p[1]"] = {"norms": lambda self, p, IS, IB: (p[1] / IS, p[1] / IB)}
    out["the integral includes the dropped events"] = {"integral": lambda self, hist, dropped: mpmath.fsum(hist) + mpmath.fsum(dropped)}

    def weights(self, p):
        w = T.weights(self, p)
        es, eb = mpmath.exp(p[0] / self.TEN), mpmath.exp(p[1] / self.TEN)
        return [[es * v for v in w[0]], [eb * v for v in w[1]]]
    out["exp(p0 / 10), exp(p1 / 10) left in the weights"] = {"weights": weights}
    out["the penalty on p[6] missing"] = {"gaussian_penalties": lambda self, p: T.gaussian_penalties(self, p)[1:]}
    out["the penalty on p[8] missing"] = {"gaussian_penalties": lambda self, p: T.gaussian_penalties(self, p)[:2]}
    out["the sign penalty missing"] = {"sign_penalty": lambda self, logl: logl}
    out["0.5 v in place of 0.5 v^2"] = {"gaussian_penalties": lambda self, p: [self.HALF * (p[6] / self.FIVE), self.HALF * p[7],
                                                                             self.HALF * p[8]]}
    out["fabs dropped from the sign penalty"] = {"sign_penalty": lambda self, logl: logl - (10 + logl)}
    return out


MUTATIONS = _mutations()


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutations_are_caught(world, name):
    """the first case and point at which the host leaves the mutated truth's bound"""
    Mutant = type("Mutant", (truth.EventTemplateTruth,), MUTATIONS[name])
    for case in world.values():
        T = Mutant(case.params, case.truth.per_event)
        for j in range(len(case.points)):
            bad = {k: v for k, v in case.ratios(T, j).items() if v > 1.0}
            if bad:
                print("%s: caught by %s, point %d: %s" % (name, case.name, j, "  ".join("%s %.3g x bound" % kv for kv in bad.items())))
                return
    pytest.fail("no case catches the mutation: " + name)
