"""The oracle's likelihoods, gradients and finite differences against the exact truth of tests/truth.py.

Every comparison is |got - exact| <= 2 (gamma_m S + extra + m eta) as tests/truth.py derives it; nothing here is a
tolerance picked by hand.  Where the IEEE evaluation of the reference's formula is not finite (overflowing products,
infinite or NaN coordinates) the class of the result is compared instead (truth.ieee_loglike says per kind what it is).

What the reference leaves open, and what the project does there:

* THardLogLikelihood.H:40-41 defines the hard likelihood "for two or more dimensions" only; its gradient functor reads
  p[1] (:73) and p[i-1] (:84) whatever the dimension, an undefined read at dim = 1.  The engines refuse Rosenbrock at
  dim < 2 with SMCMC_ERR_INVALID; oracle.hmc_gradient now refuses too (None) instead of reading outside the point.
* TDummyLogLikelihood.H:34-42 is g = -Error p, the derivative of -1/2 p^T Error p for a symmetric Error only (the true one
  is -1/2 (Error + Error^T) p).  The oracle follows the reference; test_quadform_gradient_of_a_non_symmetric_error pins
  that and shows the two differ.
"""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("smcmc_truth", os.path.join(os.path.dirname(os.path.abspath(__file__)), "truth.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

DIMS = T.DIMS
LARGE = 65             # above it the point set is thinned (exact arithmetic is slow), never the bound
KINDS = [T.ISO, T.QUADFORM, T.ROSENBROCK, T.ASYM, T.HORRIFIC, T.CONSTRAINED]
NAMES = {T.ISO: "iso", T.QUADFORM: "quadform", T.ROSENBROCK: "rosenbrock", T.ASYM: "asym", T.HORRIFIC: "horrific",
         T.CONSTRAINED: "constrained"}


valley, points, error_matrices, params_of = T.valley, T.points, T.error_matrices, T.params_of


def variants(oracle, kind):
    """(name, f(p, params) -> log L) for every arithmetic order the oracle has of this kind."""
    v = [("reference order", lambda p, prm: oracle.loglike(kind, p, prm)),
         ("fused order", lambda p, prm: oracle.loglike_order(kind, p, prm, exact=False))]
    if kind == T.QUADFORM:
        v += [("matrix-pipe rows", lambda p, prm: oracle.loglike_order(kind, p, prm, exact=False, rowwise=True)),
              ("potential from gradient", lambda p, prm: -oracle.hmc_potential(kind, p, prm, potential_from_gradient=True)),
              ("potential from fused gradient",
               lambda p, prm: -oracle.hmc_potential(kind, p, prm, potential_from_gradient=True, fused_gradient=True))]
    if kind in T.SMOOTH:
        v += [("hmc potential", lambda p, prm: -oracle.hmc_potential(kind, p, prm))]
    return v


def cases(oracle, kind, dim):
    thin = dim > LARGE
    if kind == T.QUADFORM:
        for mname, E in error_matrices(oracle, dim, thin):
            for pname, p in points(kind, dim, None, thin):
                yield "%s, %s" % (mname, pname), p, E
    else:
        for prm in params_of(oracle, kind, dim):
            for pname, p in points(kind, dim, prm, thin):
                yield pname, p, prm


def check_value(tag, got, truth):
    assert T.within(got, truth), "%s: %r vs exact %.17g, |error| = %.3g x bound (bound %.3g)" % (
        tag, got, float(truth.value), T.excess(got, truth), float(truth.bound))


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
@pytest.mark.parametrize("dim", DIMS)
def test_loglike_against_exact_truth(oracle, kind, dim):
    """Rosenbrock at dim = 1 is the empty sum, exactly 0 (THardLogLikelihood.H:60 with GetDim()-1 = 0 terms)."""
    vs = variants(oracle, kind)
    n = 0
    for name, p, prm in cases(oracle, kind, dim):
        cls = T.ieee_loglike(kind, p, prm)
        truth = T.loglike(kind, p, prm) if cls == "finite" else None
        for vname, f in vs:
            got = f(p, prm)
            tag = "%s D=%d %s, %s" % (NAMES[kind], dim, name, vname)
            if cls == "finite":
                check_value(tag, got, truth)
            elif vname == "reference order":
                assert T.classify(got) == cls, "%s: %r, IEEE evaluation of the formula gives %s" % (tag, got, cls)
            else:
                # a fused product is not rounded before the sum, so an inf - inf of the reference order may come out
                # as +-inf here; what may not happen is a finite value
                assert not np.isfinite(got) or T.classify(got) == cls, tag
            n += 1
    assert n >= 2 * len(vs)


NONFINITE = [("one inf", lambda p: _put(p, 0, np.inf)), ("one -inf", lambda p: _put(p, -1, -np.inf)),
             ("one nan", lambda p: _put(p, len(p) // 2, np.nan)), ("inf then nan", lambda p: _put(_put(p, 0, np.inf), -1, np.nan)),
             ("both infinities", lambda p: _put(_put(p, 0, np.inf), -1, -np.inf)), ("all inf", lambda p: np.full(len(p), np.inf)),
             ("squares overflow", lambda p: 1e200 * (np.abs(p) + 1)), ("1e308", lambda p: np.full(len(p), 1e308)),
             ("-1e308", lambda p: np.full(len(p), -1e308)), ("adjacent infinities", lambda p: _put(_put(p, 0, np.inf), min(1, len(p) - 1), np.inf))]


def _put(p, i, v):
    p = p.copy()
    p[i] = v
    return p


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
@pytest.mark.parametrize("dim", [1, 2, 3, 7, 64])
def test_class_of_non_finite_results(oracle, kind, dim):
    """finite / -inf / nan / the -1E+30 sentinel: the class IEEE evaluation of the reference's formula gives
    (truth.ieee_loglike writes down per kind what that is)."""
    rng = np.random.default_rng(5 + dim)
    base = rng.uniform(-0.9, 0.9, dim)
    mats = [m for _, m in error_matrices(oracle, dim)] if kind == T.QUADFORM else params_of(oracle, kind, dim)
    seen = set()
    for prm in mats:
        for name, make in NONFINITE:
            p = make(base)
            want = T.ieee_loglike(kind, p, prm)
            got = oracle.loglike(kind, p, prm)
            assert T.classify(got) == want, "%s D=%d %s: %r, expected %s" % (NAMES[kind], dim, name, got, want)
            fused = oracle.loglike_order(kind, p, prm, exact=False)
            assert (want == "finite") == bool(np.isfinite(fused) and fused != -1E+30) or T.classify(fused) == want, (name, fused, want)
            seen.add(want)
    if not (kind == T.ROSENBROCK and dim == 1):     # the empty sum: 0 whatever the point
        assert seen - {"finite"}, "the point set must reach a non-finite class"
    if kind == T.HORRIFIC:
        assert "sentinel" in seen and "nan" in seen


SMOOTH_DIMS = {T.ISO: DIMS, T.QUADFORM: DIMS, T.ROSENBROCK: DIMS[1:]}


def check_gradient(tag, got, truths):
    assert got is not None and len(got) == len(truths), tag
    worst = max(range(len(truths)), key=lambda i: T.excess(got[i], truths[i]))
    assert all(T.within(g, t) for g, t in zip(got, truths)), "%s: component %d is %r, exact %.17g, %.3g x bound" % (
        tag, worst, got[worst], float(truths[worst].value), T.excess(got[worst], truths[worst]))


def finite_gradient_cases(oracle, kind, dim):
    for name, p, prm in cases(oracle, kind, dim):
        if kind == T.QUADFORM and name.startswith("sparse") and dim > 65:
            continue
        if not np.all(np.isfinite(p)):                     # the overflowing valley: likelihood classes only
            continue
        with np.errstate(all="ignore"):
            g = oracle.hmc_gradient(kind, p, prm)
        if g is None or not np.all(np.isfinite(g)):
            assert "1e150" in name, name               # the only points whose gradient overflows
            continue
        yield name, p, prm, g


@pytest.mark.parametrize("kind", T.SMOOTH, ids=[NAMES[k] for k in T.SMOOTH])
@pytest.mark.parametrize("dim", DIMS)
def test_gradient_is_the_exact_derivative(oracle, kind, dim):
    """oracle.hmc_gradient (and the fused quadratic-form order) against the analytic derivative of the likelihood the
    truth module states, symmetric Error.  Rosenbrock at dim = 1: refused (see the module docstring)."""
    if kind == T.ROSENBROCK and dim == 1:
        assert oracle.hmc_gradient(kind, np.array([0.3])) is None
        assert oracle.hmc_potential_gradient(kind, np.array([0.3]), gradient_type=0) is None
        with pytest.raises(ValueError):
            T.gradient(kind, [0.3])
        assert oracle.loglike(kind, np.array([0.3]), [100.0]) == 0.0
        return
    n = 0
    for name, p, prm, g in finite_gradient_cases(oracle, kind, dim):
        truths = T.gradient(kind, p, prm)
        check_gradient("%s D=%d %s" % (NAMES[kind], dim, name), g, truths)
        pg = oracle.hmc_potential_gradient(kind, p, prm, gradient_type=0)          # grad U = -grad log L, exactly
        assert np.array_equal(pg, -g)
        if kind == T.QUADFORM:
            check_gradient("quadform fused D=%d %s" % (dim, name), oracle.hmc_gradient(kind, p, prm, fused=True), truths)
            if dim <= LARGE and name.endswith("gauss"):     # symmetric: the derivative of the potential itself
                true = T.true_quadform_gradient(p, prm)
                assert all(t.value == v for t, v in zip(truths, true))
        n += 1
    assert n >= 2


def test_rosenbrock_gradient_at_two_dimensions(oracle):
    """dim = 2 is the smallest the header defines: g_0 from the first-element line (:73), g_1 from the last-element line
    (:84), no middle element."""
    for p in ([0.3, -0.2], [1.0, 1.0], [1.0, np.nextafter(1.0, 2.0)], [-1.5, 2.25], [0.0, -0.0], [1e-160, 5e-324]):
        p = np.array(p)
        check_gradient("rosenbrock D=2 %r" % (p,), oracle.hmc_gradient(T.ROSENBROCK, p, [100.0]), T.gradient(T.ROSENBROCK, p, [100.0]))


@pytest.mark.parametrize("dim", [2, 3, 7, 64, 65])
def test_quadform_gradient_of_a_non_symmetric_error(oracle, dim):
    """TDummyLogLikelihood.H:34-42 walks Error(i,j) p_j while :24-28 walks Error(j,i): the functor returns -Error p, which
    is NOT the derivative -1/2 (Error + Error^T) p of the likelihood next to it unless Error is symmetric.  The reference
    only ever fills a symmetric matrix (Init(), :44-142), and the oracle and the kernels follow the functor."""
    rng = np.random.default_rng(dim)
    E = rng.standard_normal((dim, dim)) + dim * np.eye(dim)
    p = rng.standard_normal(dim)
    ref = T.gradient(T.QUADFORM, p, E)
    for fused in (False, True):
        check_gradient("non-symmetric D=%d fused=%d" % (dim, fused), oracle.hmc_gradient(T.QUADFORM, p, E, fused=fused), ref)
    g = oracle.hmc_gradient(T.QUADFORM, p, E)
    true = T.true_quadform_gradient(p, E)
    off = [abs(T.F(g[i]) - true[i]) > ref[i].bound for i in range(dim)]
    assert any(off), "-Error p equals the true derivative only for a symmetric Error"
    # the value does not care: p^T Error p = p^T Error^T p
    assert T.loglike(T.QUADFORM, p, E).value == T.loglike(T.QUADFORM, p, E.T.copy()).value
    assert T.within(oracle.loglike(T.QUADFORM, p, E), T.loglike(T.QUADFORM, p, E))
    # and the transposed walk is told apart: the test would see an oracle that indexed Error(j,i) in the gradient
    wrong = T.gradient(T.QUADFORM, p, E, transpose=True)
    assert not all(T.within(a, t) for a, t in zip(g, wrong))


FD_DIMS = {T.ISO: [1, 2, 3, 63, 64, 65], T.QUADFORM: [1, 2, 3, 16, 33], T.ROSENBROCK: [2, 3, 63, 64, 65]}


@pytest.mark.parametrize("kind", T.SMOOTH, ids=[NAMES[k] for k in T.SMOOTH])
def test_finite_difference_gradient(oracle, kind):
    """Gradient type 3 (FiniteDifferenceGradient, TSimpleHMC.H:417-444, du = 0.01) equals the central difference of the
    EXACT potential at the two doubles the reference steps to; this ties type 3 to the same truth type 0 is tied to.
    (D potentials of D or D^2 terms each in exact arithmetic: the dimensions are thinned, the bound is not.)"""
    for dim in FD_DIMS[kind]:
        rng = np.random.default_rng(dim)
        mats = [m for _, m in error_matrices(oracle, dim)] if kind == T.QUADFORM else params_of(oracle, kind, dim)
        for prm in mats:
            for name, p in (("gauss", rng.standard_normal(dim)), ("valley", valley(dim, 1.0)), ("zero", np.zeros(dim)),
                            ("1e3", 1e3 * rng.standard_normal(dim))):
                got = oracle.hmc_potential_gradient(kind, p, prm, gradient_type=3)
                truths = T.finite_difference_gradient(kind, p, prm)
                check_gradient("%s D=%d %s type 3" % (NAMES[kind], dim, name), got, truths)
                if kind == T.QUADFORM:     # the engine's association of the potential under the same differences
                    got = oracle.hmc_potential_gradient(kind, p, prm, gradient_type=3, potential_from_gradient=True)
                    check_gradient("quadform D=%d %s type 3, potential from gradient" % (dim, name), got, truths)
    assert np.array_equal(oracle.hmc_potential_gradient(T.ISO, np.ones(5), gradient_type=5), np.zeros(5))


# ---- the tests bite ---------------------------------------------------------------------------------------------------

MUT_DIMS = [2, 3, 7, 16, 31]


def _caught(oracle, kind, mutate, dims=MUT_DIMS):
    """True if the oracle's value falls outside the bound of the MUTATED truth on at least one point."""
    for dim in dims:
        for name, p, prm in cases(oracle, kind, dim):
            if T.ieee_loglike(kind, p, prm) != "finite":
                continue
            if not T.within(oracle.loglike(kind, p, prm), T.loglike(kind, p, prm, mutate=mutate)):
                return True
    return False


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
def test_a_relative_change_of_2_to_the_minus_40_is_seen(oracle, kind):
    """0.5 -> 0.5 (1 + 2^-40) (B of Rosenbrock and the slopes of asym, which carry no 0.5): seen only where the terms do
    not cancel, |value| close to S; the point set holds such a point for every kind (same-sign and Gaussian clouds)."""
    assert _caught(oracle, kind, "half")
    for dim in MUT_DIMS:       # and such a point exists at every dimension tried: |value| >= S / 2 somewhere
        ok = False
        for name, p, prm in cases(oracle, kind, dim):
            if T.ieee_loglike(kind, p, prm) == "finite":
                t = T.loglike(kind, p, prm)
                ok = ok or (t.S > 0 and abs(t.value) * 2 >= t.S)
        assert ok, (NAMES[kind], dim)


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
def test_a_sum_that_stops_one_term_early_is_seen(oracle, kind):
    assert _caught(oracle, kind, "short", [3, 7, 16, 31])


def test_gradient_mutations_are_seen(oracle):
    rng = np.random.default_rng(9)
    for dim in (3, 7, 16, 64):
        p = rng.standard_normal(dim)
        g = oracle.hmc_gradient(T.ROSENBROCK, p, [100.0])
        mutated = T.gradient(T.ROSENBROCK, p, [100.0], mutate="drop_a")
        assert not T.within(g[dim // 2], mutated[dim // 2]), "dropping -2 (1 - p_i) at i = %d of D = %d" % (dim // 2, dim)
        assert all(T.within(g[i], mutated[i]) for i in range(dim) if i != dim // 2)
        E = rng.standard_normal((dim, dim)) + dim * np.eye(dim)
        g = oracle.hmc_gradient(T.QUADFORM, p, E)
        mutated = T.gradient(T.QUADFORM, p, E, mutate="swap")
        assert not T.within(g[0], mutated[0]) and not T.within(g[dim - 1], mutated[dim - 1])
        assert all(T.within(g[i], mutated[i]) for i in range(1, dim - 1))
        short = T.gradient(T.QUADFORM, p, E, mutate="short")
        assert not any(T.within(g[i], short[i]) for i in range(dim))


# ---- the leapfrog criterion of tests/test_gpu_truth.py, on the CPU ----------------------------------------------------

class _OracleHmc:
    """oracle.HmcEnsemble behind the verbs of HmcEngine that truth.energy_ratio uses."""

    def __init__(self, oracle, dim, kind, prm, fused):
        self.h = oracle.HmcEnsemble(T.NCHAINS, dim, kind, prm, seed=T.SEED, potential_from_gradient=fused, fused_gradient=fused)

    def Start(self, x): self.h.start(x)
    def Step(self, n): self.h.step(n)
    def state(self): return self.h.state()
    def lane(self, name): return self.h.lane(name)
    def SetAlpha(self, a): self.h.set_alpha(a)
    def SetMeanEpsilon(self, e): self.h.set_mean_epsilon(e)
    def SetLeapFrog(self, n): self.h.set_leapfrog(n)


@pytest.mark.parametrize("kind,dim,eps,L,threshold", [c for c in T.LEAPFROG if c[1] <= 65],
                         ids=["%s-%d" % (NAMES[c[0]], c[1]) for c in T.LEAPFROG if c[1] <= 65])
def test_the_oracle_meets_the_leapfrog_criterion(oracle, kind, dim, eps, L, threshold):
    """The table in tests/test_gpu_truth.py: the oracle alone meets every condition, its median and share are the
    recorded ones, and the threshold is its share minus the binomial four-sigma at 200 chains."""
    prm = T.leapfrog_params(kind, dim)
    for fused in ((False, True) if kind == T.QUADFORM else (False,)):
        r = T.energy_ratio(lambda: _OracleHmc(oracle, dim, kind, prm, fused), kind, dim, prm, eps, L)
        median, share = T.judge("oracle %s D=%d fused=%d" % (NAMES[kind], dim, fused), *r, threshold)
        assert abs(median - 4.0) < 0.01
        assert abs((share - 4 * np.sqrt(share * (1 - share) / T.NCHAINS)) - threshold) < 5e-4


def _python_leapfrog(grad, q, p, eps, L):
    q, p = q.copy(), p - 0.5 * eps * grad(q)
    for i in range(L):
        q = q + eps * p
        p = p - (eps if i < L - 1 else 0.5 * eps) * grad(q)
    return q, p


def _criterion(kind, prm, grad, dim, eps, L):
    rng = np.random.default_rng(5)
    x = T.leapfrog_cloud(kind, dim, T.NCHAINS)
    m = rng.standard_normal(x.shape)
    dh = [T.energy_change(kind, prm, x, m, *_python_leapfrog(grad, x, m, e, l))[0] for e, l in ((eps, L), (eps / 2, 2 * L))]
    r = np.asarray(dh[0] / dh[1], dtype=np.float64)
    return float(np.median(r)), float(np.mean((r >= T.LO) & (r <= T.HI)))


def test_the_leapfrog_criterion_rejects_mutated_gradients():
    """A plain leapfrog with grad U of the truth's formulas passes (median 4.00, every chain inside); each single-term
    mutation leaves a first-order energy error and fails both the median and the share."""
    B = 100.0

    def rosen(q, drop=None):
        b = q[1:] - q[:-1] ** 2
        a = -2 * (1 - q[:-1])
        if drop is not None:
            a[drop] = 0
        g = np.zeros_like(q)
        g[:-1] += a - 4 * B * q[:-1] * b
        g[1:] += 2 * B * b
        return g
    E = T.spd(20)
    skew = E.copy()
    skew[0, 19] += 0.5
    skew[19, 0] -= 0.5                                    # the same quadratic form, a non-symmetric matrix

    def short(q):
        q = q.copy()
        q[-1] = 0
        return E @ q
    good = [_criterion(T.ROSENBROCK, [B], rosen, 10, 0.002, 4), _criterion(T.QUADFORM, E, lambda q: E @ q, 20, 0.05, 4)]
    bad = [_criterion(T.ROSENBROCK, [B], lambda q: rosen(q, 5), 10, 0.002, 4),         # -2 (1 - p_5) dropped
           _criterion(T.QUADFORM, skew, lambda q: skew @ q, 20, 0.05, 4),              # -Error p, Error not symmetric
           _criterion(T.QUADFORM, skew, lambda q: skew.T @ q, 20, 0.05, 4),            # the off-diagonal pair swapped
           _criterion(T.QUADFORM, E, short, 20, 0.05, 4)]                              # rows summed to D - 1
    for median, share in good:
        assert abs(median - 4.0) < 0.01 and share == 1.0, (median, share)
    for median, share in bad:
        assert not (T.LO <= median <= T.HI) and share < 0.5, (median, share)
