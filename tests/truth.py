"""Exact ground truth for the built-in likelihoods and their gradients (test helper, imported by the test modules).

Written from the reference headers' formulas, sharing no code and no floating-point order with oracle/ or the kernels:

  iso          README.md:57-66            logL = sum_i -1/2 p_i^2
  quadform     TDummyLogLikelihood.H:21-31  logL = -sum_i sum_j 1/2 p_i Error(j,i) p_j ;  :34-42  g_i = -sum_j Error(i,j) p_j
  rosenbrock   THardLogLikelihood.H:57-67   logL = -sum_{i<D-1} (1-p_i)^2 + B (p_{i+1} - p_i^2)^2 ;  :70-91 its gradient
  asym         TAsymLogLikelihood.H:20-31   logL = sum_i p_i * (p_i < 0 ? negativeSlope : positiveSlope)
  horrific     THorrificLogLikelihood.H:26-38  -1E+30 outside |p_i| <= 1, else -1/2 (sum p / sqrt(D 4/12))^2 / 0.01^2
  constrained  example4/TConstrainedLikelihood.H:26-46  -1/2 ((sum p - SV)/SC)^2 - sum_i 1/2 ((p_i - Exp_i)/Prior_i)^2

All six are rational in their inputs (the horrific one with (s / sqrt(D/3))^2 = s^2 / (D/3)), so every value here is
EXACT: doubles enter through float.as_integer_ratio(), the arithmetic is Python integers / fractions.Fraction, constants
are the exact value of the double the source spells (0.01, 0.5, 100.0, 1E+30).  Nothing is rounded before the comparison.

Every function returns a Truth(value, S, m, extra, bound):

  S      sum |t_k| over the terms the code under test adds up
  m      number of terms plus roundings per term (each function says how it counts)
  extra  first-order errors that are not proportional to a term: the rounding of p_i^2 inside b = p_{i+1} - p_i^2
         carried through 2 B |b| (Rosenbrock), the error of a long sum carried through the square it enters (horrific,
         constrained)
  bound  2 * (gamma_m S + extra + m eta),  gamma_m = m u / (1 - m u),  u = 2^-53,  eta = 2^-1074

gamma_m S is the standard bound of a serial sum of m roundings (Higham, Accuracy and Stability, section 3.1 / 4.2); it holds
for every order of summation, so it covers the reference order, the fused order (fewer roundings) and the row-wise,
butterfly and panel associations of the kernels.  m eta is the same model's absolute term for results that underflow
(eta, the smallest denormal, per rounding).  The factor 2 covers the second-order terms.  u, eta, the formula and the
factor 2 are the only constants; no tolerance here is tuned to make a test pass.
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
ETA = Fraction(1, 2 ** 1074)
HALF = Fraction(1, 2)

ISO, QUADFORM, ROSENBROCK, ASYM, HORRIFIC, CONSTRAINED = 0, 1, 2, 4, 5, 6
SMOOTH = (ISO, QUADFORM, ROSENBROCK)

Truth = namedtuple("Truth", "value S m extra bound")


def gamma(m):
    return m * U / (1 - m * U)


def F(x):
    """The exact value of a double."""
    return Fraction(*float(x).as_integer_ratio())


def _truth(value, S, m, extra=0, scale=1):
    """scale: the largest constant an underflowed intermediate is multiplied by afterwards (>= 1)."""
    bound = 2 * (gamma(m) * S + extra + m * ETA * max(1, scale))
    return Truth(value, S, m, extra, bound)


def dyadic(x):
    """Finite doubles as integers over one power of two: x_i = ints[i] / den exactly (object array, int)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if not np.all(np.isfinite(x)):
        raise ValueError("the exact truth takes finite inputs; see ieee_loglike for the rest")
    key = x.tobytes() if x.size >= 64 else None            # an Error matrix is converted once, not once per point
    if key is not None and key in _DYADIC_CACHE:
        ints, den = _DYADIC_CACHE[key]
        return ints.copy(), den
    pairs = [float(v).as_integer_ratio() for v in x]
    den = max([d for _, d in pairs] + [1])
    ints = np.empty(len(pairs), dtype=object)
    for i, (n, d) in enumerate(pairs):
        ints[i] = n * (den // d)
    if key is not None:
        _DYADIC_CACHE.clear()
        _DYADIC_CACHE[key] = (ints.copy(), den)
    return ints, den


_DYADIC_CACHE = {}


def _isum(a):
    return sum(a.tolist(), 0)


def _iabs(a):
    return np.array([abs(v) for v in a.ravel().tolist()], dtype=object).reshape(a.shape)


def within(got, truth):
    """|got - value| <= bound, in exact arithmetic; a non-finite `got` is never within."""
    got = float(got)
    if not np.isfinite(got):
        return False
    return abs(F(got) - truth.value) <= truth.bound


def excess(got, truth):
    """|got - value| / bound as a float (for messages and printed figures)."""
    got = float(got)
    if not np.isfinite(got):
        return float("inf")
    err = abs(F(got) - truth.value)
    if truth.bound == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / truth.bound)


# ---- likelihoods -----------------------------------------------------------------------------------------------------
# mutate: one single-term change of the truth-side formula, for the sensitivity checks of tests/test_truth_cpu.py
#   "half"   0.5 -> 0.5 (1 + 2^-40)  (Rosenbrock and asym carry no 0.5: B, and the slopes, take the factor)
#   "short"  the sum stops one term early
MUT_HALF = 1 + Fraction(1, 2 ** 40)


def iso(p, mutate=None):
    """m = D + 2: one rounding in (-0.5 p) p, one in the accumulation."""
    P, d = dyadic(p)
    if mutate == "short":
        P = P[:-1]
    s = _isum(P * P)
    h = HALF * (MUT_HALF if mutate == "half" else 1)
    S = HALF * Fraction(s, d * d)
    return _truth(-h * Fraction(s, d * d), S, len(P) + 2)


def quadform(p, error, mutate=None):
    """t_ij = 1/2 p_i Error(j,i) p_j, D^2 terms.  m = D^2 + 4: three multiplications and the accumulation per term in the
    reference order; the potential-from-gradient and matrix-pipe associations (row sums of Error p, then 1/2 p_i s_i
    summed over i) put 2 D + 3 <= D^2 + 4 roundings on a term."""
    P, d = dyadic(p)
    n = len(P)
    E, de = dyadic(error)
    E = E.reshape(n, n)
    if mutate == "short":
        P = P.copy()
        P[-1] = 0
    v = _isum(P * np.dot(E.T, P)) if n else 0
    s = _isum(_iabs(P) * np.dot(_iabs(E).T, _iabs(P))) if n else 0
    h = HALF * (MUT_HALF if mutate == "half" else 1)
    den = d * d * de
    return _truth(-h * Fraction(v, den), HALF * Fraction(s, den), n * n + 4)


def rosenbrock(p, b=100.0, mutate=None):
    """t_i = (1-p_i)^2 + B b_i^2, b_i = p_{i+1} - p_i^2.  m = (D-1) + 7: a (1), a a (1), p p (1, its absolute part is in
    `extra`), the subtraction (1, counted twice through the square), B b (1), (B b) b (1), the inner sum (1), the
    accumulation.  extra = sum_i 2 B |b_i| u p_i^2 + B (u p_i^2)^2."""
    P, d = dyadic(p)
    n = len(P)
    B = F(b) * (MUT_HALF if mutate == "half" else 1)
    last = n - 1 - (1 if mutate == "short" else 0)
    if last <= 0:
        return _truth(Fraction(0), Fraction(0), 7)
    P0, P1 = P[:last], P[1:last + 1]
    A = d - P0                       # a = A / d
    Bn = P1 * d - P0 * P0            # b = Bn / d^2
    sa, sb = _isum(A * A), _isum(Bn * Bn)
    value = Fraction(sa, d * d) + B * Fraction(sb, d ** 4)
    carried = _isum(_iabs(Bn) * P0 * P0)                    # sum |b_i| p_i^2 * d^4
    sq = _isum(P0 * P0 * P0 * P0)                           # sum p_i^4 * d^4
    extra = 2 * abs(B) * U * Fraction(carried, d ** 4) + abs(B) * U * U * Fraction(sq, d ** 4)
    return _truth(-value, value if B >= 0 else Fraction(sa, d * d) - B * Fraction(sb, d ** 4), last + 7, extra, abs(B))


def asym(p, positive=-1.0, negative=100.0, mutate=None):
    """t_i = slope p_i.  m = D + 2."""
    P, d = dyadic(p)
    if mutate == "short":
        P = P[:-1]
    pos, neg = F(positive), F(negative)
    if mutate == "half":
        pos, neg = pos * MUT_HALF, neg * MUT_HALF
    v, s = Fraction(0), Fraction(0)
    for x in P.tolist():
        t = Fraction(x, d) * (neg if x < 0 else pos)        # -0.0 and +0.0 are not < 0: positiveSlope, value 0 either way
        v += t
        s += abs(t)
    return _truth(v, s, len(P) + 2, 0, max(abs(pos), abs(neg)))


def horrific(p, mutate=None):
    """Inside the box V = -1/2 s^2 / (D/3) / sigma^2 with s = sum p, sigma the double 0.01.  The sum's error
    gamma_D sum|p| enters through the square, 2 |s| ds <= 2 T ds with T = sum|p| >= |s|, and eight roundings follow
    it (4/12 D, sqrt counted twice through the square, the division twice, the product, two divisions by sigma): every
    product p_i p_j goes through the sum twice, so S = c T^2 and m = 2 D + 8."""
    P, d = dyadic(p)
    n = len(P)
    if any(abs(x) > d for x in P.tolist()):
        return _truth(-F(1E+30), F(1E+30), 0)
    Q = P[:-1] if mutate == "short" else P
    s, T = Fraction(_isum(Q), d), Fraction(_isum(_iabs(Q)), d)
    sigma = F(0.01)
    c = (HALF * (MUT_HALF if mutate == "half" else 1)) / Fraction(n * 4, 12) / sigma / sigma
    return _truth(-c * s * s, HALF / Fraction(n * 4, 12) / sigma / sigma * T * T, 2 * n + 8, 0, 1 / (sigma * sigma))


def constrained(p, params, mutate=None):
    """t_0 = 1/2 w^2, w = (sum p - SV) / SC; t_i = 1/2 v_i^2, v_i = (p_i - Exp_i) / Prior_i.  m = (D + 1) + 6 (the
    subtraction and the division twice each through the square, 0.5 v, (0.5 v) v, the accumulation).  extra: the error
    of the D-term sum, dw = gamma_D sum|p| / |SC|, carried through the square: |w| dw + dw^2 / 2."""
    P, d = dyadic(p)
    n = len(P)
    prm = [F(v) for v in np.asarray(params, dtype=np.float64).ravel()]
    sv, sc, exp, prior = prm[0], prm[1], prm[2:2 + n], prm[2 + n:2 + 2 * n]
    h = HALF * (MUT_HALF if mutate == "half" else 1)
    w = (Fraction(_isum(P), d) - sv) / sc
    dw = gamma(n) * Fraction(_isum(_iabs(P)), d) / abs(sc)
    value = h * w * w
    S = HALF * w * w
    last = n - (1 if mutate == "short" else 0)
    for i in range(last):
        v = (Fraction(P[i], d) - exp[i]) / prior[i]
        value += h * v * v
        S += HALF * v * v
    return _truth(-value, S, n + 1 + 6, abs(w) * dw + dw * dw / 2)


def loglike(kind, p, params=None, mutate=None):
    if kind == ISO:
        return iso(p, mutate)
    if kind == QUADFORM:
        return quadform(p, params, mutate)
    if kind == ROSENBROCK:
        return rosenbrock(p, 100.0 if params is None else np.ravel(params)[0], mutate)
    if kind == ASYM:
        prm = (-1.0, 100.0) if params is None else tuple(np.ravel(params)[:2])
        return asym(p, prm[0], prm[1], mutate)
    if kind == HORRIFIC:
        return horrific(p, mutate)
    if kind == CONSTRAINED:
        return constrained(p, params, mutate)
    raise ValueError(kind)


def potential(kind, p, params=None):
    t = loglike(kind, p, params)
    return Truth(-t.value, t.S, t.m, t.extra, t.bound)


# ---- gradients of log L ----------------------------------------------------------------------------------------------
# mutate: "drop_a" drops the -2 (1 - p_i) term of the middle Rosenbrock index D // 2; "swap" exchanges Error(0, D-1) and
# Error(D-1, 0); "short" sums the quadratic form's rows to D - 1.

def gradient(kind, p, params=None, mutate=None, transpose=False):
    """A list of Truth, one per component.  QUADFORM is the reference's g_i = -sum_j Error(i,j) p_j
    (TDummyLogLikelihood.H:34-42); transpose=True walks Error(j,i) instead, as the likelihood does (what the functor must NOT do, see tests/test_truth_cpu.py)."""
    P, d = dyadic(p)
    n = len(P)
    if kind == ISO:                                        # d/dp (-p^2 / 2) = -p: no rounding at all
        return [_truth(-Fraction(x, d), abs(Fraction(x, d)), 0) for x in P.tolist()]
    if kind == QUADFORM:
        E, de = dyadic(params)
        E = E.reshape(n, n)
        if transpose:
            E = E.T
        if mutate == "swap":
            E = E.copy()
            E[0, n - 1], E[n - 1, 0] = E[n - 1, 0], E[0, n - 1]
        Q = P.copy()
        if mutate == "short":
            Q[-1] = 0
        v = np.dot(E, Q)
        s = np.dot(_iabs(E), _iabs(Q))
        # m = D + 1: the product and the accumulation
        return [_truth(-Fraction(v[i], d * de), Fraction(s[i], d * de), n + 1) for i in range(n)]
    if kind == ROSENBROCK:
        if n < 2:
            raise ValueError("THardLogLikelihood.H:40-41: defined for two or more dimensions")
        B = F(100.0 if params is None else np.ravel(params)[0])
        x = [Fraction(v, d) for v in P.tolist()]
        b = [x[i + 1] - x[i] * x[i] for i in range(n - 1)]
        out = []
        for i in range(n):
            terms, extra = [], Fraction(0)
            if i < n - 1:                                   # from t_i: 2 (1 - p_i) + 4 B p_i b_i
                if not (mutate == "drop_a" and i == n // 2):
                    terms.append(2 * (1 - x[i]))
                terms.append(4 * B * x[i] * b[i])
                extra += 4 * B * abs(x[i]) * U * x[i] * x[i]
            if i > 0:                                       # from t_{i-1}: -2 B b_{i-1}
                terms.append(-2 * B * b[i - 1])
                extra += 2 * B * U * x[i - 1] * x[i - 1]
            # m = 3 terms + 7 roundings (1 - p, p p, the subtraction, 4 B, (4 B) p, its product with b, the accumulation)
            out.append(_truth(sum(terms), sum(abs(t) for t in terms), 10, extra, 4 * B))
        return out
    raise ValueError("no gradient functor for kind %d" % kind)


def true_quadform_gradient(p, error):
    """d/dp of -1/2 p^T Error p = -1/2 (Error + Error^T) p, exact (list of Fraction)."""
    P, d = dyadic(p)
    n = len(P)
    E, de = dyadic(error)
    E = E.reshape(n, n)
    v = np.dot(E + E.T, P)
    return [-HALF * Fraction(v[i], d * de) for i in range(n)]


def finite_difference_gradient(kind, p, params=None, du=0.01):
    """FiniteDifferenceGradient (TSimpleHMC.H:417-444) of the exact potential: the two points are the doubles the
    reference steps to (work[i] -= du; work[i] += 2.0 * du, one rounding each), the potential at them is exact, and
    grad_i = 0.5 (U2 - U1) / du.  bound: the two potentials' bounds through 0.5 / du, plus gamma_3 |grad_i| for the
    subtraction, the product and the division."""
    p = np.asarray(p, dtype=np.float64)
    out = []
    fdu = F(du)
    for i in range(p.size):
        w = p.copy()
        w[i] = w[i] - du
        u1 = potential(kind, w, params)
        w[i] = w[i] + 2.0 * du
        u2 = potential(kind, w, params)
        value = HALF * (u2.value - u1.value) / fdu
        extra = (u1.bound + u2.bound) / 2 * HALF / fdu      # the bounds carry the factor 2 already: halve, _truth doubles
        out.append(_truth(value, abs(value), 3, extra))
    return out


# ---- IEEE evaluation of the reference's formulas (non-finite inputs) -------------------------------------------------

def ieee_loglike(kind, p, params=None):
    """The reference's formula statement by statement in IEEE doubles (Python floats: no exceptions from + - * /), for the
    CLASS of the result only: 'finite', '-inf', '+inf', 'nan', or 'sentinel' (-1E+30).  Per kind:
      iso          nan if any p is nan, else -inf if any |p| is inf or p^2 overflows, else finite
      quadform     inf * 0 = nan, so one infinite coordinate gives nan through every zero of Error; overflowing products
                   give +-inf and their mixture nan
      rosenbrock   p_i = +-inf: b = p_{i+1} - inf, b^2 = inf, -inf unless p_{i+1} = +inf too (inf - inf = nan)
      asym         +-inf by the slopes' signs, nan from nan or from +inf and -inf terms meeting
      horrific     |p| > 1 (inf included) is the sentinel; nan compares false, joins the sum and gives nan
      constrained  nan from nan, else -inf from any infinity unless infinities of both signs meet in the sum (nan)"""
    p = [float(v) for v in np.ravel(p)]
    n = len(p)
    if kind == ISO:
        v = 0.0
        for x in p:
            v += -0.5 * x * x
    elif kind == QUADFORM:
        E = np.asarray(params, dtype=np.float64).reshape(n, n)
        v = 0.0
        for i in range(n):
            for j in range(n):
                v -= 0.5 * p[i] * float(E[j, i]) * p[j]
    elif kind == ROSENBROCK:
        B = 100.0 if params is None else float(np.ravel(params)[0])
        v = 0.0
        for i in range(n - 1):
            a = 1.0 - p[i]
            b = p[i + 1] - p[i] * p[i]
            v -= a * a + B * b * b
    elif kind == ASYM:
        pos, neg = (-1.0, 100.0) if params is None else [float(t) for t in np.ravel(params)[:2]]
        v = 0.0
        for x in p:
            v += x * (neg if x < 0.0 else pos)
    elif kind == HORRIFIC:
        v = 0.0
        for x in p:
            if abs(x) > 1.0:
                return "sentinel"
            v += x
        v /= float(np.sqrt(n * 4.0 / 12.0))
        v = -0.5 * v * v / 0.01 / 0.01
    elif kind == CONSTRAINED:
        prm = [float(t) for t in np.ravel(params)]
        s = 0.0
        for x in p:
            s += x
        s = (s - prm[0]) / prm[1]
        v = 0.0
        v -= 0.5 * s * s
        for i in range(n):
            t = (p[i] - prm[2 + i]) / prm[2 + n + i]
            v -= 0.5 * t * t
    else:
        raise ValueError(kind)
    return classify(v)


def classify(v):
    v = float(v)
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "-inf" if v < 0 else "+inf"
    return "sentinel" if v == -1E+30 else "finite"


# ---- the point set (shared by tests/test_truth_cpu.py and tests/test_gpu_truth.py) ----------------------------------

# the tiling edges, and the largest dimension of every register-array size of the build (SMCMC_FOR_EACH_DP: 7 15 31 47 50
# 63) with the smallest of the next
DIMS = [1, 2, 3, 7, 8, 15, 16, 31, 32, 47, 48, 50, 51, 63, 64, 65, 128, 129, 256, 257, 511, 512]


def ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def valley(dim, start, ks=(0, -1, 0, -2, -1)):
    """The Rosenbrock valley p[i+1] = p[i]^2 (1 + k u), k a small integer: b = p[i+1] - p[i]^2 cancels to the last bits.
    Squaring doubles the distance from 1 at every step: with k <= 0 the point leaves 1 downwards after some 50
    coordinates and runs through every magnitude down to the denormals and 0; with k > 0 it overflows."""
    p = np.empty(dim)
    p[0] = start
    with np.errstate(over="ignore"):     # a start above 1 leaves the doubles after some 60 squarings: those points
        for i in range(dim - 1):         # are compared by class, like every other non-finite one
            p[i + 1] = ulps(p[i] * p[i], ks[i % len(ks)])
    return p


def points(kind, dim, params, thin=False):
    rng = np.random.default_rng(1000 * kind + dim)
    g = rng.standard_normal(dim)
    pts = [("gauss", g), ("1e3", 1e3 * g)]
    if kind == HORRIFIC:
        pts += [("inside", rng.uniform(-1, 1, dim)), ("same sign", rng.uniform(0.1, 1, dim))]
    if kind == CONSTRAINED:
        pts += [("near expected", params[2:2 + dim] + 0.1 * g)]
    if thin:
        return pts
    pts += [("valley 1", valley(dim, 1.0)), ("valley 0.5", valley(dim, 0.5)), ("valley 1+", valley(dim, ulps(1.0, 3), (0, 1, -1, 2, -3))),
            ("1e-160", 1e-160 * g), ("1e-8", 1e-8 * g), ("1e150", 1e150 * g), ("same sign", np.abs(g) + 0.5),
            ("+0", np.zeros(dim)), ("-0", -np.zeros(dim)), ("denormal", np.full(dim, 5e-324)),
            ("-denormal", np.full(dim, -5e-324)), ("mixed zeros", np.where(np.arange(dim) % 2, -0.0, 5e-324))]
    if kind == HORRIFIC:
        edge = np.where(np.arange(dim) % 2, -1.0, 1.0)
        out = np.ones(dim)
        out[dim // 2] = np.nextafter(1.0, 2.0)
        pts += [("box edge", edge), ("box corner", np.ones(dim)), ("one ulp outside", out), ("one ulp outside, negative", -out)]
    if kind == CONSTRAINED:
        pts += [("expected", params[2:2 + dim].copy())]
    return pts


def error_matrices(oracle, dim, thin=False):
    rng = np.random.default_rng(77 + dim)
    a = rng.standard_normal((dim, dim))
    spd = a @ a.T / dim + np.eye(dim)
    spd = 0.5 * (spd + spd.T)
    out = [("header", oracle.dummy_error_matrix(dim)[1])]     # entries ~5e5 cancelling to O(1) on the pair (0, D-1)
    if not thin:
        out.append(("spd", spd))
    if not thin and dim >= 2:
        cov = np.eye(dim)
        cov[0, dim - 1] = cov[dim - 1, 0] = 0.5
        sp = np.linalg.inv(cov)
        sp[np.abs(sp) < 1e-12] = 0.0
        out.append(("sparse", 0.5 * (sp + sp.T)))              # identity plus one pair: the kernels' sparse walk
    return out


def params_of(oracle, kind, dim):
    if kind == ROSENBROCK:
        return [np.array([100.0])]
    if kind == ASYM:
        return [np.array([-1.0, 100.0])]
    if kind == CONSTRAINED:
        return [oracle.constrained_params(dim)]
    return [None]


# ---- extended precision for many points at large dimensions ---------------------------------------------------------

def quadform_longdouble(X, error):
    """The quadratic form for the columns of X[dim][n] in np.longdouble (64-bit significand): (value[n], bound[n]) with
    bound = 2 (gamma_m(u) S + m eta) for the code under test, as quadform() has it, plus the truth's own error
    2 gamma_m(2^-64) S."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not the x87 extended format here"
    X = np.asarray(X, dtype=np.longdouble)
    E = np.asarray(error, dtype=np.longdouble)
    n = X.shape[0]
    value = -0.5 * np.einsum("ic,ic->c", X, E.T @ X)
    S = 0.5 * np.einsum("ic,ic->c", np.abs(X), np.abs(E).T @ np.abs(X))
    m = n * n + 4
    g = float(gamma(m)) + m * 2.0 ** -64 / (1 - m * 2.0 ** -64)
    return value, 2 * (g * S * np.longdouble(1 + 2.0 ** -50) + m * np.longdouble(2.0) ** -1074)     # + m eta, as _truth()


# ---- the leapfrog energy-error criterion (tests/test_gpu_truth.py on the device, tests/test_truth_cpu.py on the oracle) ----

LO, HI = 4 * (0.9 / 1.1) ** 2, 4 * (1.1 / 0.9) ** 2
NCHAINS = 200
SEED = 20240607


def potential_ld(kind, Q, prm):
    """U = -log L of the columns of Q[dim][n] from the truth's formulas in np.longdouble, with the rounding bound of this
    evaluation (gamma_m(2^-64) S, doubled)."""
    Q = np.asarray(Q, dtype=np.longdouble)
    dim = Q.shape[0]
    if kind == ISO:
        u = 0.5 * np.sum(Q * Q, axis=0)
        S, m = u, dim + 2
    elif kind == QUADFORM:
        E = np.asarray(prm, dtype=np.longdouble)
        u = 0.5 * np.einsum("ic,ic->c", Q, E.T @ Q)
        S, m = 0.5 * np.einsum("ic,ic->c", np.abs(Q), np.abs(E).T @ np.abs(Q)), dim * dim + 4
    else:
        B = np.longdouble(np.ravel(prm)[0])
        a = 1 - Q[:-1]
        b = Q[1:] - Q[:-1] * Q[:-1]
        u = np.sum(a * a + B * b * b, axis=0)
        S, m = u + 2 * B * np.sum(np.abs(b) * Q[:-1] * Q[:-1], axis=0), dim + 7
    return u, 2 * (m * 2.0 ** -64) * S


def energy_change(kind, prm, q0, p0, q1, p1):
    u0, b0 = potential_ld(kind, q0, prm)
    u1, b1 = potential_ld(kind, q1, prm)
    k0 = 0.5 * np.sum(np.asarray(p0, np.longdouble) ** 2, axis=0)
    k1 = 0.5 * np.sum(np.asarray(p1, np.longdouble) ** 2, axis=0)
    dim = q0.shape[0]
    rounding = b0 + b1 + 2 * (dim + 2) * 2.0 ** -64 * (k0 + k1)
    return (u1 + k1) - (u0 + k0), rounding


def leapfrog_cloud(kind, dim, n):
    rng = np.random.default_rng(1234 + dim)
    if kind == ROSENBROCK:
        return 1.0 + 0.02 * rng.standard_normal((dim, n))
    return rng.standard_normal((dim, n))


def energy_ratio(make, kind, dim, prm, eps, L):
    """make() -> an engine with Start/Step/state/lane/SetAlpha/SetMeanEpsilon/SetLeapFrog.  Returns the per-chain ratio
    dH(eps, L) / dH(eps/2, 2L), the mask of chains that count, and the shares left out."""
    X = leapfrog_cloud(kind, dim, NCHAINS)
    dh, keep_all, rejected, small = [], np.ones(NCHAINS, bool), 0.0, 0.0
    for e_, l_ in ((eps, L), (eps / 2, 2 * L)):
        h = make()
        h.Start(X)
        h.Step(1)                                   # every chain now holds a momentum of its own
        q0, p0 = h.state()[:2]
        h.SetAlpha(1.0)
        h.SetMeanEpsilon(-e_)
        h.SetLeapFrog(l_)
        h.Step(1)
        q1, p1 = h.state()[:2]
        acc = np.asarray(h.lane("last_accept")).astype(bool)
        d, rounding = energy_change(kind, prm, q0, p0, q1, p1)
        dh.append(d)
        rejected = max(rejected, 1.0 - acc.mean())
        keep_all &= acc
        if e_ != eps:
            tiny = np.abs(d) < 100 * rounding
            small = float(np.mean(tiny & acc))
            keep_all &= ~tiny
    with np.errstate(all="ignore"):
        ratio = np.asarray(dh[0] / dh[1], dtype=np.float64)
    return ratio, keep_all, rejected, small


def judge(tag, ratio, keep, rejected, small, threshold):
    assert rejected <= 0.01, "%s: %.3f of the chains rejected" % (tag, rejected)
    assert small <= 0.05, "%s: %.3f of the chains below 100 x the rounding of dH" % (tag, small)
    r = ratio[keep]
    median, share = float(np.median(r)), float(np.mean((r >= LO) & (r <= HI)))
    print("%s: rejected %.3f, small %.3f, median ratio %.3f, share inside %.3f (threshold %.3f)" % (tag, rejected, small, median, share, threshold))
    assert LO <= median <= HI, "%s: median ratio %.3f" % (tag, median)
    assert share >= threshold, "%s: %.3f of the chains in [%.2f, %.2f], threshold %.3f" % (tag, share, LO, HI, threshold)
    return median, share


# (kind, dim, eps, L, threshold = oracle's share - 4 sigma binomial at 200 chains), see the module docstring
LEAPFROG = [(ISO, 20, 0.05, 4, 1.000), (ISO, 63, 0.05, 4, 0.962), (QUADFORM, 20, 0.05, 4, 1.000),
            (ROSENBROCK, 10, 0.002, 4, 1.000), (ISO, 64, 0.05, 4, 1.000), (QUADFORM, 64, 0.05, 4, 1.000),
            (QUADFORM, 129, 0.05, 4, 1.000), (QUADFORM, 512, 0.02, 4, 1.000), (ROSENBROCK, 65, 0.002, 4, 1.000)]


def spd(dim, seed=77):
    """A random symmetric positive definite Error."""
    rng = np.random.default_rng(seed + dim)
    a = rng.standard_normal((dim, dim))
    m = a @ a.T / dim + np.eye(dim)
    return 0.5 * (m + m.T)


def leapfrog_params(kind, dim):
    if kind == QUADFORM:
        return spd(dim)
    return np.array([100.0]) if kind == ROSENBROCK else None
