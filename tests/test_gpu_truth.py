"""Device likelihoods and the HMC leapfrog against the exact truth of tests/truth.py, not via the oracle.

Likelihood values: every built-in kind at every dimension of the CPU list (truth.DIMS) on every engine, one adversarial
point per chain; what an engine does not serve is asserted to be refused with its documented status.
|device - exact| <= 2 (gamma_m S + extra + m eta) (tests/truth.py); at dim > 65 the quadratic form's truth is
np.longdouble with its own error term added (truth.quadform_longdouble).  Where an oracle variant of the same
arithmetic order exists the device value is also one of the oracle's, bit for bit.

Leapfrog energy error (test_leapfrog_energy_error_is_second_order).  With SetAlpha(1.0) a step is a deterministic
leapfrog from the state HmcEngine.state() shows, so dH = U(q1) + |p1|^2/2 - U(q0) - |p0|^2/2 with U from the truth
(extended precision) must fall fourfold when eps is halved and L doubled: per chain the ratio lies in
[4 (0.9/1.1)^2, 4 (1.1/0.9)^2] = [2.68, 5.98] from the +-10 % jitter of epsilon alone.  A gradient that is not the
derivative of U leaves a first-order term: the ratio goes to 2 or changes sign.  eps, L, the start cloud and the seed
were chosen on the CPU with oracle.HmcEnsemble (same alpha, epsilon, leapfrog), which gave, with 200 chains:

  case             eps    L  rejected  below 100 x rounding  median ratio  share in [2.68, 5.98]  threshold
  iso D=20         0.05   4  0.000     0.000                 4.001         1.000                  1.000
  iso D=63         0.05   4  0.000     0.000                 4.002         0.990                  0.962
  quadform D=20    0.05   4  0.000     0.000                 4.001         1.000                  1.000
  rosenbrock D=10  0.002  4  0.000     0.000                 4.001         1.000                  1.000
  iso D=64         0.05   4  0.000     0.000                 4.002         1.000                  1.000
  quadform D=64    0.05   4  0.000     0.000                 4.001         1.000                  1.000
  quadform D=129   0.05   4  0.000     0.000                 4.001         1.000                  1.000
  quadform D=512   0.02   4  0.000     0.000                 4.000         1.000                  1.000
  rosenbrock D=65  0.002  4  0.000     0.000                 4.002         1.000                  1.000

(quadform: a random symmetric positive definite Error, spd(dim); the same figures with the oracle's fused gradient and
potential-from-gradient association.)  threshold = the oracle's share minus 4 sqrt(s (1 - s) / 200), the binomial
four-sigma at that chain count; a share of 1.000 leaves no allowance.  The medians sit at 4.00 rather than anywhere in the
interval because both runs key the epsilon draw on the same (seed, chain, step): the jitter is the same in both.
eps L <= 0.2 is far below a quarter orbit (pi/2 at unit curvature; 0.008 against ~0.05 at the Rosenbrock curvature
~1e3), so the reversal test of LeapFrog does not cut the trajectory.

tests/test_truth_cpu.py keeps both halves of this honest without a device: test_the_oracle_meets_the_leapfrog_criterion
reproduces the table (the cases up to D = 65) through the same energy_ratio / judge of tests/truth.py, and
test_the_leapfrog_criterion_rejects_mutated_gradients runs a plain Python leapfrog with mutated gradients: true gradients
give medians 4.00 and shares 1.000; Rosenbrock with the -2 (1 - p_5) term dropped median 2.44, share 0.385; -Error p of
a non-symmetric Error 1.00 / 0.010; one off-diagonal pair swapped 1.00 / 0.010; rows summed to D - 1 1.00 / 0.000.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("smcmc_truth", os.path.join(os.path.dirname(os.path.abspath(__file__)), "truth.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

NAMES = {T.ISO: "iso", T.QUADFORM: "quadform", T.ROSENBROCK: "rosenbrock", T.ASYM: "asym", T.HORRIFIC: "horrific",
         T.CONSTRAINED: "constrained"}
INVALID, RUNTIME, UNSUPPORTED = 1, 3, 5      # SMCMC_ERR_*


def like_params(oracle, kind, dim, which="header"):
    if kind == T.QUADFORM:
        return dict(T.error_matrices(oracle, dim))[which]
    return T.params_of(oracle, kind, dim)[0]


def start_cloud(kind, dim, nchains, prm):
    """X[dim][nchains]: one adversarial point of the CPU point set per chain where Start admits it (finite, log L above
    -0.999999E+10), Gaussian clouds of several scales on the rest."""
    rng = np.random.default_rng(31 * dim + kind)
    pts = []
    for name, p in T.points(kind, dim, prm):
        if np.all(np.isfinite(p)) and T.ieee_loglike(kind, p, prm) == "finite" and "1e150" not in name:
            if float(T.loglike(kind, p, prm).value) > -1e9:
                pts.append(p)
    scales = [1.0, 1e-3, 0.3, 3.0]
    while len(pts) < nchains:
        s = scales[len(pts) % len(scales)]
        if kind == T.HORRIFIC:
            pts.append(rng.uniform(-1, 1, dim) * min(s, 1.0))
        elif kind == T.CONSTRAINED:
            pts.append(prm[2:2 + dim] + s * rng.standard_normal(dim))
        elif kind == T.ROSENBROCK:
            pts.append(1.0 + 0.05 * s * rng.standard_normal(dim))
        else:
            pts.append(s * rng.standard_normal(dim))
    return np.ascontiguousarray(np.array(pts[:nchains]).T)


def check_values(tag, got, X, kind, prm):
    """Every chain's value against the truth of its own point."""
    dim, n = X.shape
    assert got.shape == (n,)
    if kind == T.QUADFORM and dim > 65:
        value, bound = T.quadform_longdouble(X, prm)
        err = np.abs(got.astype(np.longdouble) - value)
        bad = np.flatnonzero(~(err <= bound))
        assert bad.size == 0, "%s: chain %d is %r, truth %r, %.3g x bound" % (tag, bad[0], got[bad[0]], value[bad[0]], err[bad[0]] / bound[bad[0]])
        return float(np.max(err / bound))
    worst = 0.0
    for c in range(n):
        t = T.loglike(kind, X[:, c], prm)
        assert T.within(got[c], t), "%s: chain %d is %r, exact %.17g, %.3g x bound" % (tag, c, got[c], float(t.value), T.excess(got[c], t))
        worst = max(worst, T.excess(got[c], t))
    return worst


def oracle_values(oracle, X, kind, prm):
    """Every value some arithmetic order of the oracle gives for each chain's point: [variant][chain]."""
    n = X.shape[1]
    fs = [lambda p: oracle.loglike(kind, p, prm), lambda p: oracle.loglike_order(kind, p, prm, exact=False)]
    if kind == T.QUADFORM:
        fs += [lambda p: oracle.loglike_order(kind, p, prm, exact=False, rowwise=True),
               lambda p: -oracle.hmc_potential(kind, p, prm, potential_from_gradient=True),
               lambda p: -oracle.hmc_potential(kind, p, prm, potential_from_gradient=True, fused_gradient=True)]
    return np.array([[f(X[:, c]) for c in range(n)] for f in fs])


def in_oracle(got, ov):
    return np.all(np.any(ov == got[None, :], axis=0))


# ---- likelihood at chosen points ----------------------------------------------------------------------------------------
# Every kind at every dimension of the CPU list on every engine; what an engine does not serve is asserted to be refused
# with its documented status.  Every cell runs all of an engine's configurations (arithmetic order, mode, dense / sparse
# quadratic form, per-chain kernel), except the HMC engine's four, of which a cell runs two (which two turns with the
# dimension) and all four at the FULL dimensions.

DIMS = T.DIMS
KINDS = [T.ISO, T.QUADFORM, T.ROSENBROCK, T.ASYM, T.HORRIFIC, T.CONSTRAINED]
CELLS = [(k, d) for k in KINDS for d in DIMS]
CELL_IDS = ["%s-%d" % (NAMES[k], d) for k, d in CELLS]
FULL = (7, 63, 64, 129)
NCHAINS = 70             # 64 and a ragged tail: padded lanes exist
_cells = {}


class Cell:
    """One (kind, dim): the parameters, one adversarial point per chain, the truth of every chain's point (computed once)
    and, up to dim 129, the values the oracle's arithmetic orders give."""

    def __init__(self, oracle, kind, dim, nchains=NCHAINS):
        self.kind, self.dim, self.n = kind, dim, nchains
        i = DIMS.index(dim)
        which = ("header", "sparse", "spd")[i % 3] if dim >= 2 else "header"
        self.prm = like_params(oracle, kind, dim, which)
        self.X = start_cloud(kind, dim, nchains, self.prm)
        if kind == T.QUADFORM and dim > 65:
            self.ld = T.quadform_longdouble(self.X, self.prm)
        else:
            self.ld = None
            self.truths = [T.loglike(kind, self.X[:, c], self.prm) for c in range(nchains)]
        self.ov = oracle_values(oracle, self.X, kind, self.prm) if dim <= 129 else None

    def check(self, tag, got, bits):
        """bits: "reference" (the oracle's reference order, bit for bit), "any" (one of the oracle's orders), None."""
        tag = "%s D=%d %s" % (NAMES[self.kind], self.dim, tag)
        assert got.shape == (self.n,), tag
        if self.ld is not None:
            value, bound = self.ld
            err = np.abs(got.astype(np.longdouble) - value)
            bad = np.flatnonzero(~(err <= bound))
            assert bad.size == 0, "%s: chain %d is %r, truth %r, %.3g x bound" % (tag, bad[0], got[bad[0]], value[bad[0]], err[bad[0]] / bound[bad[0]])
        else:
            for c, t in enumerate(self.truths):
                assert T.within(got[c], t), "%s: chain %d is %r, exact %.17g, %.3g x bound" % (tag, c, got[c], float(t.value), T.excess(got[c], t))
        if self.ov is not None and bits == "reference":
            assert np.array_equal(got, self.ov[0]), tag + ": not the oracle's reference order"
        elif self.ov is not None and bits == "any":
            assert in_oracle(got, self.ov), tag + ": no arithmetic order of the oracle gives these bits"


def cell(oracle, kind, dim):
    if (kind, dim) not in _cells:
        _cells[(kind, dim)] = Cell(oracle, kind, dim)
    return _cells[(kind, dim)]


def rotate(configs, dim, keep):
    """All configurations at the FULL dimensions, else `keep` of them, starting where the dimension's index points."""
    if dim in FULL:
        return list(configs)
    i = DIMS.index(dim)
    return [configs[(i + j * (len(configs) // keep)) % len(configs)] for j in range(keep)]


def refused(gpu, status, make):
    with pytest.raises(gpu.SmcmcError) as err:
        e = make()
        e.close()
    assert err.value.status == status, err.value


@pytest.mark.parametrize("kind,dim", CELLS, ids=CELL_IDS)
def test_metropolis_start_likelihood(gpu, oracle, kind, dim):
    """Engine.Start(x0[dim][nchains]) -> lane("logl"): FROZEN and POOLED, both arithmetic orders, the sparse walk of the
    quadratic form and the dense sum."""
    if kind == T.ROSENBROCK and dim < 2:          # THardLogLikelihood.H:40-41
        return refused(gpu, INVALID, lambda: gpu.Engine(dim, NCHAINS, likelihood=kind))
    cl = cell(oracle, kind, dim)
    configs = [(gpu.MODE_FROZEN, True, 0.0), (gpu.MODE_POOLED, True, 1.0), (gpu.MODE_POOLED, False, 0.0), (gpu.MODE_FROZEN, False, 1.0)]
    if kind == T.QUADFORM:
        configs += [(m, x, 1.0 - d) for m, x, d in configs]
    for mode, exact, dense in configs:
        e = gpu.Engine(dim, NCHAINS, likelihood=kind, likelihood_params=cl.prm, mode=mode, exact=exact)
        if kind == T.QUADFORM:
            e.set_param("DENSE_QUADFORM", dense)
        assert e.Start(cl.X)
        got = e.lane("logl")
        e.close()
        cl.check("mode=%d exact=%d dense=%s" % (mode, exact, dense), got, "reference" if exact else "any")


def test_metropolis_start_likelihood_with_two_ragged_blocks(gpu, oracle):
    for kind, dim in ((T.QUADFORM, 63), (T.ROSENBROCK, 65)):
        cl = Cell(oracle, kind, dim, 130)
        for exact in (True, False):
            e = gpu.Engine(dim, 130, likelihood=kind, likelihood_params=cl.prm, exact=exact)
            assert e.Start(cl.X)
            cl.check("130 chains exact=%d" % exact, e.lane("logl"), "reference" if exact else "any")
            e.close()


@pytest.mark.parametrize("kind,dim", [(T.ROSENBROCK, 7), (T.HORRIFIC, 31), (T.QUADFORM, 7), (T.ISO, 65), (T.ROSENBROCK, 129)],
                         ids=lambda v: str(v))
def test_forced_step_likelihood(gpu, oracle, kind, dim):
    """ForceStep(points) then Step(1, metropolis=2): the step kernel's own likelihood of the forced proposal
    (logl_proposed), including the points Start refuses: below -0.999999E+10, the -1E+30 sentinel, non-finite."""
    prm = like_params(oracle, kind, dim)
    n = 70
    X = start_cloud(kind, dim, n, prm)
    X[:, 3] = 1e150 * np.sign(X[:, 3] + 0.5)       # overflows, or far outside the box
    X[0, 5] = np.inf
    X[dim - 1, 6] = np.nan
    X[:, 7] = 1e5 * (1 + np.arange(dim) % 3)       # finite, far below the bad-start threshold for the smooth kinds
    if kind == T.HORRIFIC:
        X[:, 8] = 1.0
        X[dim // 2, 8] = np.nextafter(1.0, 2.0)
    for mode in (gpu.MODE_FROZEN, gpu.MODE_POOLED):
        for exact in (True, False):
            e = gpu.Engine(dim, n, likelihood=kind, likelihood_params=prm, mode=mode, exact=exact)
            assert e.Start(np.full(dim, 0.5))
            e.ForceStep(X)
            e.Step(1, metropolis=2)
            got = e.lane("logl_proposed")
            e.close()
            for c in range(n):
                cls = T.ieee_loglike(kind, X[:, c], prm)
                tag = "%s D=%d mode=%d exact=%d chain %d" % (NAMES[kind], dim, mode, exact, c)
                if cls == "finite":
                    t = T.loglike(kind, X[:, c], prm)
                    assert T.within(got[c], t), "%s: %r, exact %.17g, %.3g x bound" % (tag, got[c], float(t.value), T.excess(got[c], t))
                elif exact:
                    assert T.classify(got[c]) == cls, "%s: %r, expected %s" % (tag, got[c], cls)
                else:
                    assert not np.isfinite(got[c]) or T.classify(got[c]) == cls, tag



@pytest.mark.parametrize("kind,dim", CELLS, ids=CELL_IDS)
def test_per_chain_start_likelihood(gpu, oracle, kind, dim):
    """SMCMC_MODE_PER_CHAIN: the wave kernel, the per-lane kernel (SMCMC_P_PERCHAIN_WAVE = 0) up to dim 63, the workgroup
    kernel up to smcmc_max_perchain_dim(); beyond, SMCMC_ERR_UNSUPPORTED.  Reference-order arithmetic only."""
    dmax = gpu.load().smcmc_max_perchain_dim()
    if kind == T.ROSENBROCK and dim < 2:
        return refused(gpu, INVALID, lambda: gpu.Engine(dim, NCHAINS, likelihood=kind, mode=gpu.MODE_PER_CHAIN))
    if dim > 63:
        refused(gpu, UNSUPPORTED, lambda: gpu.Engine(dim, NCHAINS, likelihood=kind, mode=gpu.MODE_PER_CHAIN))
    if dim > dmax:
        return refused(gpu, UNSUPPORTED, lambda: gpu.Engine(dim, NCHAINS, likelihood=kind, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True))
    cl = cell(oracle, kind, dim)
    configs = [(1.0, False), (0.0, False), (None, True)] if dim <= 63 else [(None, True)]
    for wave, wg in configs:
        e = gpu.Engine(dim, NCHAINS, likelihood=kind, likelihood_params=cl.prm, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=wg)
        if wave is not None:
            e.set_param("PERCHAIN_WAVE", wave)
        assert e.Start(cl.X)
        got = e.lane("logl")
        e.close()
        cl.check("per chain wave=%s workgroup=%s" % (wave, wg), got, "reference")


def test_per_chain_refuses_the_fused_order_and_serves_its_largest_dimension(gpu, oracle):
    dmax = gpu.load().smcmc_max_perchain_dim()
    with pytest.raises(gpu.SmcmcError) as err:
        e = gpu.Engine(7, NCHAINS, mode=gpu.MODE_PER_CHAIN, exact=False)
        e.Start(np.zeros(7))
    assert err.value.status == UNSUPPORTED
    for kind in (T.ISO, T.QUADFORM, T.ROSENBROCK):
        prm = like_params(oracle, kind, dmax, "spd")
        X = start_cloud(kind, dmax, NCHAINS, prm)
        e = gpu.Engine(dmax, NCHAINS, likelihood=kind, likelihood_params=prm, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)
        assert e.Start(X)
        check_values("workgroup %s D=%d" % (NAMES[kind], dmax), e.lane("logl"), X, kind, prm)
        e.close()


@pytest.mark.parametrize("kind,dim", CELLS, ids=CELL_IDS)
def test_vaat_start_likelihood(gpu, oracle, kind, dim):
    if kind == T.ROSENBROCK and dim < 2:
        return refused(gpu, INVALID, lambda: gpu.VaatEngine(dim, NCHAINS, likelihood=kind))
    cl = cell(oracle, kind, dim)
    for exact in (True, False):
        e = gpu.VaatEngine(dim, NCHAINS, likelihood=kind, likelihood_params=cl.prm, exact=exact)
        assert e.Start(cl.X) is not False
        got = e.lane("logl")
        e.close()
        cl.check("vaat exact=%d" % exact, got, "reference" if exact else "any")


@pytest.mark.parametrize("kind,dim", CELLS, ids=CELL_IDS)
def test_hmc_start_potential(gpu, oracle, kind, dim):
    """HmcEngine.Start: logl = -potential for every built-in kind (the stress kinds are HMC targets through gradient
    types 2 / 3 / 5), both arithmetic orders (the matrix-pipe potential among them), POOLED and PER_CHAIN."""
    if kind == T.ROSENBROCK and dim < 2:
        return refused(gpu, INVALID, lambda: gpu.HmcEngine(dim, NCHAINS, likelihood=kind))
    cl = cell(oracle, kind, dim)
    configs = [(gpu.MODE_POOLED, True), (gpu.MODE_PER_CHAIN, True), (gpu.MODE_PER_CHAIN, False), (gpu.MODE_POOLED, False)]
    for mode, exact in rotate(configs, dim, 2):
        h = gpu.HmcEngine(dim, NCHAINS, likelihood=kind, likelihood_params=cl.prm, exact=exact, mode=mode)
        h.Start(cl.X)
        got = h.state()[2]
        if kind >= T.ASYM and dim in FULL and mode == gpu.MODE_POOLED and exact:
            with pytest.raises(gpu.SmcmcError) as err:       # no gradient functor (TSimpleHMC.H:85-89): type 0 is refused
                h.Step(1)
            assert err.value.status == RUNTIME
        h.close()
        cl.check("hmc mode=%d exact=%d" % (mode, exact), got, "any")


def test_engines_refuse_what_they_do_not_serve(gpu):
    refused(gpu, UNSUPPORTED, lambda: gpu.HmcEngine(513, 64))
    refused(gpu, UNSUPPORTED, lambda: gpu.Engine(513, 64))
    refused(gpu, UNSUPPORTED, lambda: gpu.VaatEngine(513, 64))
    for make in (gpu.Engine, gpu.VaatEngine, gpu.HmcEngine):      # THardLogLikelihood.H:40-41: two or more dimensions
        refused(gpu, INVALID, lambda: make(1, 64, likelihood=T.ROSENBROCK))


# ---- leapfrog energy error ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dim,eps,L,threshold", T.LEAPFROG, ids=["%s-%d" % (NAMES[c[0]], c[1]) for c in T.LEAPFROG])
def test_leapfrog_energy_error_is_second_order(gpu, kind, dim, eps, L, threshold):
    prm = T.leapfrog_params(kind, dim)
    configs = [(True, gpu.MODE_POOLED), (False, gpu.MODE_POOLED), (True, gpu.MODE_PER_CHAIN)]
    for exact, mode in configs:
        def make():
            return gpu.HmcEngine(dim, T.NCHAINS, likelihood=kind, likelihood_params=prm, seed=T.SEED, exact=exact, mode=mode)
        tag = "%s D=%d exact=%d mode=%d" % (NAMES[kind], dim, exact, mode)
        T.judge(tag, *T.energy_ratio(make, kind, dim, prm, eps, L), threshold)
