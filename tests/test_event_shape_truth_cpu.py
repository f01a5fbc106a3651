"""SMCMC_LIKE_EVENT_SHAPE on the host (smcmc_event_shape_evaluate) against the definition in high precision
(tests/event_shape_truth.py), without a GPU.  The device kernels are held to the host bit for bit elsewhere
(tests/test_gpu_event_shape*.py), so this is what says that the value they all agree on is the right one.

The notation and the bounds of a class weight, a bin's content, an integral, a normalisation, the expectation, a bin
term and the sign and Gaussian penalties are those of tests/test_event_template_truth_cpu.py and
tests/test_event_sample_truth_cpu.py: u = 2^-53; E_exp, E_log, E_atan the largest errors of smcmc_exp, smcmc_log and
smcmc_atan in ulp of the true value; everything first order in u and multiplied by 1 + 2^-20.  What is new:

THE FIXTURES.  Every evaluation used here has a decision gap (event_shape_truth.py: the cuts, the histogram split, the bin
edges, the shape's segment and its clamps) of at least GAP = 1e-9 and at least 1000 times the derived bound of every
corrected mass, asserted with the truth alone.  The samples are event_shape_ref.make_sample's with the masses that sit
exactly on a centre moved off it (on_centres=False): a centre is a rounded quantity on the host and a real one in the
truth, and a mass on it would decide its segment within the gap.  No case is skipped.

THE TAG FRACTION takes p / 10: the quotient is rounded (u relative, so at most |p / 10| u in the tangent's sum, which
the sum's own rounding bound u |s| covers together with it when written 2 u in place of u): c_w of the template's file
with (2 + 2 E_atan) replaced by (3 + 2 E_atan).

A CENTRE on the host, low + i bw + 0.5 bw with bw = (high - low) / n: the difference and the quotient round (2 u of bw),
the product i bw (u), the two sums (u each of a value of at most H = max(|low|, |high|)): |dc| <= 6 u H.

THE SHAPE's value v = y[k] + dx s, dx = x - c[k], s = (y[k + 1] - y[k]) / (c[k + 1] - c[k]):
  y = p / 10                u |y|
  dx                        dc + u |dx|
  D = c[k + 1] - c[k]       2 dc + u |D| absolute, r_D = 2 dc / D + u relative
  N = y[k + 1] - y[k]       u (|y[k]| + |y[k + 1]|) + u |N|
  s = N / D                 ds = (u (|y[k]| + |y[k + 1]|) + u |N|) / D + |s| (r_D + u)
  dx s                      |s| (dc + u |dx|) + |dx| ds + u |dx s|
  v                         dv = u |y[k]| + the line above + u |v|;   a clamped event: dv = u |y[k]|
and the event's weight r exp(v): relative c_w u + dv + 2 E_exp u + u -- c_e = c_w + dv / u + 2 E_exp + 1 in place of c_w
in the bound of a bin's content.

THE INTEGRAL joins four histograms: m = 4 nbins + 3.

A SHAPE PENALTY sum_i sum_j (y[i] y[j]) Kinv[i][j], Kinv the library's own doubles: each term carries the two roundings
of y and its two products, 4 u |term|; the n^2 terms are added by n^2 - 1 roundings:
    dpen = (4 u + gamma_(n^2 - 1)) sum |term|,   and L' = L - pen:  e' = e + dpen + u |L'|.

THE INVERSE.  For example3's two kernels max |K Kinv - I|, the product in mpmath, is at most n 2^-53 cond_1(K): a
sanity bound of the elimination, not a measurement (numpy's LU inverse gives 3e-11 and 4e-9 against 4e-9 and 8e-7).

THE MUTATIONS.  test_mutations_are_caught applies each of them to a copy of the truth and requires that the host leaves
a bound at some case and point; the one mutation that the likelihood cannot see -- the signal's fixed zeros left out of
the penalty -- is put to smcmc_event_shape_gp_penalty with a vector whose end values are not zero.
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


sref, truth, sample_test = _load("event_shape_ref"), _load("event_shape_truth"), _load("test_event_sample_truth_cpu")

U = sample_test.U
SECOND_ORDER = sample_test.SECOND_ORDER
GAP = sample_test.GAP
E_EXP, E_LOG, E_ATAN = sample_test.E_EXP, sample_test.E_LOG, sample_test.E_ATAN
NPOINTS = 12
CASES = {"197ev_50bins": (60, 137, 50, 201), "64ev_5bins": (30, 34, 5, 202), "65ev_59bins": (25, 40, 59, 207)}


def gamma(m):
    return m * U / (1 - m * U)


# ---- the bounds of the docstring ----------------------------------------------------------------------------------
def weight_constants(T, p):
    """c_w[background][tagged]"""
    E = T.per_event
    out = []
    for tangent, shift in zip((E.tan_fakes, E.tan_efficiency), T.tag_shifts(p)):
        c = E.corrected_probability(tangent, shift)
        q = abs(c - T.HALF)
        out.append([(q * (3 + 2 * E_ATAN) + c) / (1 - c) + 3, (q / c) * (3 + 2 * E_ATAN) + 2])
    return out


def shape_error(T, p, r, i):
    """dv / u of event i"""
    background = T.background[i]
    low, high, n = T.ranges[background]
    y = T.control_values(p)[background]
    c = T.centres(background)
    k, clamped = r.located[i]
    if clamped:
        return abs(y[k])
    dc = 6 * max(abs(low), abs(high))
    x = T.raw_mass[i]
    dx, D, N = x - c[k], c[k + 1] - c[k], y[k + 1] - y[k]
    s = N / D
    r_d = 2 * dc / D + 1
    ds = ((abs(y[k]) + abs(y[k + 1])) + abs(N)) / D + abs(s) * (r_d + 1)
    return abs(y[k]) + abs(s) * (dc + abs(dx)) + abs(dx) * ds + abs(dx * s) + abs(r.shape[i])


def bounds(T, p, r):
    """{"S", "B": relative per bin, "IS", "IB", "ws", "wb": relative, "mc": absolute per bin, "penB", "penS", "logl": absolute}"""
    rows = 4 * T.nbins
    cw = weight_constants(T, p)
    n = [[0] * rows, [0] * rows]
    worst = [[mpf(0)] * rows, [mpf(0)] * rows]
    for i, (k, background, tagged) in enumerate(zip(r.where, T.background, T.tagged)):
        if k >= 0:
            n[background][k] += 1
            worst[background][k] = max(worst[background][k], cw[background][tagged] + shape_error(T, p, r, i) + 2 * E_EXP + 1)
    rel = [[(n[c][k] - 1 + worst[c][k]) * U if n[c][k] else mpf(0) for k in range(rows)] for c in range(2)]
    r_i = [max(rel[c]) + gamma(rows + 3) for c in range(2)]
    r_w = [v + U for v in r_i]
    dmc = [abs(r.ws * r.S[k]) * (r_w[0] + rel[0][k] + U) + abs(r.wb * r.B[k]) * (r_w[1] + rel[1][k] + U) + U * abs(r.mc[k])
           for k in range(rows)]
    total, size = mpf(0), mpf(0)
    for d, mc, dm, term in zip(T.data, r.mc, dmc, r.terms):
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
    for t in (T.HALF * (p[3] / T.FIVE) ** 2, T.HALF * p[4] ** 2, T.HALF * p[5] ** 2):
        value = value - t
        e = e + 3 * U * t + U * abs(value)
    y = T.control_values(p)
    dpen = []
    for background in (1, 0):
        yy, kinv = y[background], T.kinv[background]
        m = len(yy)
        size = mpmath.fsum(abs(yy[i] * yy[j] * kinv[i][j]) for i in range(m) for j in range(m))
        dpen.append((4 * U + gamma(m * m - 1)) * size)
    for pen, d in zip((r.penB, r.penS), dpen):
        value = value - pen
        e = e + d + U * abs(value)
    s = SECOND_ORDER
    return {"S": [v * s for v in rel[0]], "B": [v * s for v in rel[1]], "IS": r_i[0] * s, "IB": r_i[1] * s,
            "ws": r_w[0] * s, "wb": r_w[1] * s, "mc": [v * s for v in dmc], "penB": dpen[0] * s, "penS": dpen[1] * s,
            "logl": e * s}


def _ratio(got, want, bound):
    err = abs(mpf(float(got)) - want)
    if err == 0:
        return 0.0
    return float(err / bound) if bound > 0 else math.inf


class Case:
    """one sample: its points, the host's values at them, the truth"""
    def __init__(self, name, oracle, smcmc):
        nsig, nbkg, nbins, key = CASES[name]
        self.name = name
        self.params = sref.make_sample(oracle, nsig, nbkg, nbins, key, on_centres=False)
        self.points = sref.points(oracle, NPOINTS, key + 1000, self.params)
        self.host = [smcmc.event_shape_evaluate(self.params, p, histograms=True, parts=True) for p in self.points]
        self.kinv = (self.host[0][2]["KinvB"], self.host[0][2]["KinvS"])
        self.truth = truth.EventShapeTruth(self.params, *self.kinv)
        self.results = [self.truth.evaluate(p) for p in self.points]

    def ratios(self, T, j, r=None):
        """{stage: worst error / bound} of the host at point j, judged by the truth T"""
        with mpmath.workprec(truth.PREC):
            r = r or T.evaluate(self.points[j])
            p = [mpf(float(v)) for v in self.points[j]]
            b = bounds(T, p, r)
            logl, hist, parts = self.host[j]
            out = {}
            for key, want in (("S", r.S), ("B", r.B)):
                out[key] = max(_ratio(g, w, bd * w) for g, w, bd in zip(parts[key].ravel(), want, b[key]))
            for key, want in (("IS", r.IS), ("IB", r.IB), ("ws", r.ws), ("wb", r.wb)):
                out[key] = _ratio(parts[key], want, b[key] * abs(want))
            out["mc"] = max(_ratio(g, w, bd) for g, w, bd in zip(hist.ravel(), r.mc, b["mc"]))
            out["penB"] = _ratio(parts["penB"], r.penB, b["penB"])
            out["penS"] = _ratio(parts["penS"], r.penS, b["penS"])
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
    T = case.truth
    E = T.per_event
    worst_mass = 0.0
    with mpmath.workprec(truth.PREC):
        for point, r in zip(case.points, case.results):
            p9 = [mpf(float(v)) for v in T.systematics([float(v) for v in point])]
            bound = max(float(sample_test.mass_bound(E, p9, i)) for i in range(E.nevents))
            worst_mass = max(worst_mass, bound)
            assert float(r.gap) >= GAP and float(r.gap) >= 1000.0 * bound
    smallest = min(float(r.gap) for r in case.results)
    print("%s: smallest decision gap over %d points %.3e, largest bound of a corrected mass %.3e"
          % (case.name, len(case.points), smallest, worst_mass))
    # what the mutations need: every kind of segment in both classes, a negative count of either class, all four
    # histograms of both classes, points off the origin
    kinds = {(b, "clamp" if c else "line") for (k, c), b in zip(case.results[0].located, T.background)}
    assert kinds == {(False, "clamp"), (False, "line"), (True, "clamp"), (True, "line")}
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
            p = [mpf(float(v)) for v in case.points[j]]
            b = bounds(case.truth, p, r)
            y = case.truth.control_values(p)
            size = mpmath.fsum(abs(t) for t in r.terms)
            for background in (0, 1):
                kinv = case.truth.kinv[background]
                size += mpmath.fsum(abs(y[background][i] * y[background][k] * kinv[i][k]) for i in range(len(kinv)) for k in range(len(kinv)))
            assert b["logl"] <= 1e-12 * (10 + size)


def test_exp_and_log_at_this_likelihoods_arguments(world, smcmc):
    """E_exp where the shape takes an exponential, E_log at mc / data"""
    args = np.unique([float(a) for c in world.values() for r in c.results for a in r.log_args])
    with mpmath.workprec(128):
        err = sample_test._ulp_errors(smcmc.selftest_detmath(0, args, device=-1), [mpmath.log(mpf(float(v))) for v in args])
    print("smcmc_log at %d arguments mc / data: largest error %.4f ulp of the true value" % (args.size, err.max()))
    assert err.max() <= E_LOG
    args = np.unique([float(a) for c in world.values() for r in c.results for a in r.exp_args])
    with mpmath.workprec(128):
        err = sample_test._ulp_errors(smcmc.selftest_detmath(1, args, device=-1), [mpmath.exp(mpf(float(v))) for v in args])
    print("smcmc_exp at %d shape values: largest error %.4f ulp of the true value" % (args.size, err.max()))
    assert err.max() <= E_EXP


def test_the_inverse_of_example3s_kernels(smcmc):
    """max |K Kinv - I| in mpmath against n 2^-53 cond_1(K), cond_1 from mpmath's own inverse"""
    kb, ks = sref.example3_kernels()
    data = np.ones((4, 5))
    events = np.array([[135.0, 0, 20.0, 0, 135.0, 40.5], [320.0, 2, 150.0, 1, 320.0, 96.0]])
    params = smcmc.event_shape_params(events, data, 5, 0.0, 500.0, kernel_b=kb, kernel_s=ks)
    _, parts = smcmc.event_shape_evaluate(params, np.zeros(31), parts=True)
    with mpmath.workprec(truth.PREC):
        for name, k, kinv in (("background", kb, parts["KinvB"]), ("signal", ks, parts["KinvS"])):
            n = len(k)
            K = mpmath.matrix([[mpf(float(v)) for v in row] for row in k])
            V = mpmath.matrix([[mpf(float(v)) for v in row] for row in kinv])
            R = K * V - mpmath.eye(n)
            residual = max(abs(R[i, j]) for i in range(n) for j in range(n))
            cond = mpmath.mnorm(K, 1) * mpmath.mnorm(K ** -1, 1)
            bound = n * U * cond
            print("%s kernel: max |K Kinv - I| %.3e, n u cond_1 %.3e (cond_1 %.3e)" % (name, float(residual), float(bound), float(cond)))
            assert residual <= bound
            assert np.array_equal(kinv, kinv.T) or float(max(abs(V[i, j] - V[j, i]) for i in range(n) for j in range(n))) <= float(bound * mpmath.mnorm(V, 1))


def _mutations():
    T = truth.EventShapeTruth
    out = {}
    out["example2's parameter order"] = {
        "systematics": lambda self, p: [0.0, 0.0, p[2], p[3], p[4], p[5], p[6], 0.0, 0.0],
        "tag_shifts": lambda self, p: (p[7] / self.TEN, p[8] / self.TEN)}
    out["the / 10 in the arctangent dropped"] = {"tag_shifts": lambda self, p: (p[4], p[5])}
    out["VeryClose merged into Close"] = {
        "histogram_of": lambda self, sep, tagged: 3 if tagged else 1 if sep < self.cut_close else 2}
    out["the integral without VeryClose"] = {"integral": lambda self, hist: mpmath.fsum(hist[self.nbins:])}
    out["the shape read at the corrected mass"] = {"shape_argument": lambda self, raw, corrected: corrected}
    out["the signal control values unshifted"] = {
        "control_values": lambda self, p: [[p[20 + i] / self.TEN for i in range(11)] + [mpf(0), mpf(0)], T.control_values(self, p)[1]]}

    def always_b(self, x, c, low, high):
        n = len(c)
        return min(min(int(mpmath.floor(n * (x - low) / (high - low))), n - 1), n - 2)
    out["k = b always"] = {"segment": always_b}
    out["a penalty's sign"] = {"apply_shape_penalty": lambda self, logl, pen: logl + pen}
    out["K used for Kinv"] = {"penalty": lambda self, y, background: truth.gp_penalty(y, self.kernel[background])}
    return out


MUTATIONS = _mutations()


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutations_are_caught(world, name):
    """the first case and point at which the host leaves the mutated truth's bound"""
    Mutant = type("Mutant", (truth.EventShapeTruth,), MUTATIONS[name])
    for case in world.values():
        T = Mutant(case.params, *case.kinv)
        for j in range(len(case.points)):
            try:
                ratios = case.ratios(T, j)
            except (ZeroDivisionError, IndexError):
                continue                     # (a mutant that leaves a class empty or the table at this point proves nothing)
            bad = {k: v for k, v in ratios.items() if v > 1.0}
            if bad:
                print("%s: caught by %s, point %d: %s" % (name, case.name, j, "  ".join("%s %.3g x bound" % kv for kv in bad.items())))
                return
    pytest.fail("no case catches the mutation: " + name)


def test_mutation_end_points_left_out_of_the_penalty(world, smcmc):
    """smcmc_event_shape_gp_penalty on the signal's kernel with a vector whose end values are not zero: within the
    penalty's bound of the truth, and outside it when the truth leaves the end points out"""
    case = world["197ev_50bins"]
    ks = np.ascontiguousarray(sref.split(case.params)["KS"])
    y = np.array([0.3, -0.1, 0.2, 0.05, -0.25, 0.15, 0.1, -0.05, 0.2, -0.15, 0.1, 0.05, -0.2])
    lib, C, dp = smcmc.load(), smcmc._capi.C, smcmc._capi._dp
    pen, inv = C.c_double(0.0), np.zeros((13, 13))
    assert lib.smcmc_event_shape_gp_penalty(ks.ctypes.data_as(dp), 13, y.ctypes.data_as(dp), C.byref(pen), inv.ctypes.data_as(dp)) == 0
    assert np.array_equal(inv, case.kinv[1])
    with mpmath.workprec(truth.PREC):
        yy = [mpf(float(v)) for v in y]
        kinv = [[mpf(float(v)) for v in row] for row in inv]
        want = truth.gp_penalty(yy, kinv)
        size = mpmath.fsum(abs(yy[i] * yy[j] * kinv[i][j]) for i in range(13) for j in range(13))
        bound = (2 * U + gamma(168)) * size * SECOND_ORDER          # (y enters exactly here: two products a term)
        inner = truth.gp_penalty(yy[1:12], [row[1:12] for row in kinv[1:12]])
        print("penalty of a vector with non-zero ends: error / bound %.3f; without the end points %.3g x bound"
              % (_ratio(pen.value, want, bound), _ratio(pen.value, inner, bound)))
        assert _ratio(pen.value, want, bound) <= 1.0
        assert _ratio(pen.value, inner, bound) > 1.0
