"""HMC with the caller's own gradient on the device (the OptionalGradient of TSimpleHMC<UserLikelihood, OptionalGradient>,
TSimpleHMC.H:79-89, 467-532; BadGrad.C): a gradient compiled in with a user likelihood (smcmc_user_gradient_at,
examples/user_likelihood_quadgrad.hip.h -> libsmcmc_amd_user_grad.so) and a gradient matrix given to the built-in
quadratic form at run time (smcmc_hmc_set_gradient_matrix)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from hmc_gradient_ref import HmcGradientRef  # noqa: E402
from hmc_user_gradient_cases import (ASYM_HEADER, ASYM_LIB, STAT_CHAINS, STAT_DIM, STAT_EPS, STAT_LEAP, STAT_MAX_CURVATURE, STAT_SEED,  # noqa: E402
                                     STAT_STEPS, badgrad_matrices, grad_lib, spd_matrix, stat_bounds_hold, stat_start_points)

pytestmark = pytest.mark.gpu

SEED = 31
EPS, LEAP = 0.1, 4


def _shape_boundary():
    """The largest dimension the four-wavefront shape of hmc_step_kernel serves (smcmc_hmc_create: W = 4 up to
    4 * kPanelCW, 8 above), read from the source so that the cases stay on both sides of it."""
    text = open(os.path.join(ROOT, "root-simple-mcmc_amd", "csrc", "smcmc_panel_kernel.hip.h")).read()
    return 4 * int(re.search(r"constexpr int kPanelCW = (\d+);", text).group(1))


W4_MAX = _shape_boundary()
# at most 63, just above 63, the last dimension of the four-wavefront shape, an odd one of the eight-wavefront shape
USER_DIMS = [5, 64, W4_MAX, W4_MAX + 3]
NCHAINS = 70     # one full wavefront of chains and a partial one


def _two_matrices(error, gradient):
    return np.concatenate([np.asarray(error).ravel(), np.asarray(gradient).ravel()])


def _start_points(dim, n, seed=0):
    return np.random.default_rng(1000 + dim + seed).uniform(-1.0, 1.0, size=(dim, n))


_ORACLE_CHAINS = {}


def _fixed_oracle_chains(oracle, dim, gradient_type, steps=6):
    """oracle.Hmc(LIKE_QUADFORM, potential_from_gradient=False) for every chain, computed once per (dim, gradient type):
    (q, momentum, logl, naccept) after `steps` fixed steps."""
    key = (dim, gradient_type, steps)
    if key not in _ORACLE_CHAINS:
        err = spd_matrix(dim, dim)
        x0 = _start_points(dim, NCHAINS)
        q = np.zeros((dim, NCHAINS)); m = np.zeros((dim, NCHAINS)); logl = np.zeros(NCHAINS)
        nacc = np.zeros(NCHAINS, np.int32)
        for c in range(NCHAINS):
            h = oracle.Hmc(dim, kind=oracle.LIKE_QUADFORM, params=err, seed=SEED, chain_id=c, potential_from_gradient=False)
            h.set_gradient_type(gradient_type)
            h.start(x0[:, c])
            h.set_mean_epsilon(-EPS); h.set_leapfrog(LEAP)
            for _ in range(steps):
                h.step()
                nacc[c] += int(h.scalars["last_accept"])
            q[:, c], m[:, c], logl[c] = h.accepted, h.momentum, -h.scalars["accepted_potential"]
        _ORACLE_CHAINS[key] = (q, m, logl, nacc)
    return _ORACLE_CHAINS[key]


def _user_engine(gpu, dim, n, err, grad, **kw):
    return gpu.HmcEngine(dim, n, likelihood=gpu.LIKE_USER, likelihood_params=_two_matrices(err, grad), seed=SEED,
                         library=grad_lib(gpu), **kw)


# ---- 5. the compiled-in gradient against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("gradient_type", [0, 1, 4])
@pytest.mark.parametrize("dim", USER_DIMS)
def test_user_gradient_fixed_step_is_the_reference_chain(gpu, oracle, dim, gradient_type):
    """G = Error: every chain of the user library is oracle.Hmc on the quadratic form in the reference's own summation
    order (TDummyLogLikelihood.H:24-27 for the potential, :34-42 for the gradient), bit for bit, through both workgroup
    shapes and a partial wavefront of chains.  Two launches of three steps: the many-steps-per-launch path."""
    err = spd_matrix(dim, dim)
    e = _user_engine(gpu, dim, NCHAINS, err, err)
    assert e.has_gradient
    e.Start(_start_points(dim, NCHAINS))
    e.SetMeanEpsilon(-EPS); e.SetLeapFrog(LEAP)
    e.SetGradientType(gradient_type)
    e.Step(3); e.Step(3)
    q, m, logl = e.state()
    oq, om, ologl, onacc = _fixed_oracle_chains(oracle, dim, 0)
    assert np.array_equal(q, oq) and np.array_equal(m, om)
    assert np.array_equal(logl, ologl)
    assert np.array_equal(e.lane("naccept"), onacc)
    assert np.all(e.lane("trials") == 6) and 0 < onacc.sum()


@pytest.mark.parametrize("dim", [5, 64])
def test_user_gradient_library_still_runs_finite_differences(gpu, oracle, dim):
    """Type 3 on the same library is the finite-difference chain (TSimpleHMC.H:417-444), not the user's gradient."""
    err = spd_matrix(dim, dim)
    e = _user_engine(gpu, dim, NCHAINS, err, err)
    e.Start(_start_points(dim, NCHAINS))
    e.SetMeanEpsilon(-EPS); e.SetLeapFrog(LEAP)
    e.Step(2, gradient_type=3)
    q, m, logl = e.state()
    oq, om, ologl, onacc = _fixed_oracle_chains(oracle, dim, 3, steps=2)
    assert np.array_equal(q, oq) and np.array_equal(m, om) and np.array_equal(logl, ologl)
    assert np.array_equal(e.lane("naccept"), onacc)
    fq = _fixed_oracle_chains(oracle, dim, 0, steps=2)[0] if dim == 5 else None
    assert fq is None or not np.array_equal(q, fq)      # and the two gradients do differ in the last bits


# ---- 6. the same library with the reference's default tuning --------------------------------------------------------
@pytest.mark.parametrize("dim", [5, 70])
def test_user_gradient_with_pooled_tuning(gpu, oracle, dim):
    n, steps = 70, 12
    err = spd_matrix(dim, dim)
    e = _user_engine(gpu, dim, n, err, err)
    o = oracle.HmcEnsemble(n, dim, kind=oracle.LIKE_QUADFORM, params=err, seed=SEED, group=e.moment_group, sync_every=1,
                           potential_from_gradient=False)
    x0 = np.ones(dim)
    e.Start(x0); o.start(x0)
    for chunk in (1, steps - 1):
        e.Step(chunk); o.step(chunk)
        q, m, logl = e.state()
        oq, om = o.state()
        assert np.array_equal(q, oq) and np.array_equal(m, om)
        assert np.array_equal(logl, -o.lane("accepted_potential"))
        assert np.array_equal(e.lane("mean_epsilon"), o.lane("mean_epsilon"))
        assert np.array_equal(e.lane("leapfrog"), o.lane("leapfrog_steps").astype(np.int32))
        assert np.array_equal(e.lane("reversal_len"), o.lane("reversal_len"))
        assert np.array_equal(e.lane("acceptance"), o.lane("current_acceptance"))
        for name in ("trace", "orbit", "updates", "cov_trials"):
            assert e.tuning[name] == o.shared[name], name
    assert e.lane("naccept").sum() > 0


@pytest.mark.parametrize("dim", [5, 70])
def test_user_gradient_with_every_chain_tuning_itself(gpu, oracle, dim):
    n, steps = 70, 12
    err = spd_matrix(dim, dim)
    e = _user_engine(gpu, dim, n, err, err, mode=gpu.MODE_PER_CHAIN)
    x0 = np.ones(dim)
    e.Start(x0)
    e.Step(steps)
    q, m, logl = e.state()
    lanes = {k: e.lane(k) for k in ("mean_epsilon", "leapfrog", "reversal_len", "acceptance")}
    for c in (0, 1, 63, 64, n - 1):
        h = oracle.Hmc(dim, kind=oracle.LIKE_QUADFORM, params=err, seed=SEED, chain_id=c, potential_from_gradient=False)
        h.start(x0)
        h.run(steps)
        s = h.scalars
        assert np.array_equal(q[:, c], h.accepted) and np.array_equal(m[:, c], h.momentum), c
        assert logl[c] == -s["accepted_potential"]
        assert lanes["mean_epsilon"][c] == s["mean_epsilon"] and lanes["leapfrog"][c] == s["leapfrog_steps"]
        assert lanes["reversal_len"][c] == s["reversal_len"] and lanes["acceptance"][c] == s["current_acceptance"]
    assert e.lane("naccept").sum() > 0


# ---- 7. a gradient matrix equal to Error changes nothing -----------------------------------------------------------
LANES = ("logl", "logl_proposed", "acceptance", "naccept", "last_accept", "trials", "mean_epsilon", "leapfrog",
         "reversal_len", "contributes")


def _same_engines(a, b, tag):
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y), tag
    for name in LANES:
        assert np.array_equal(a.lane(name), b.lane(name)), f"{tag}: {name}"


@pytest.mark.parametrize("mode", ["fixed", "pooled", "per_chain"])
@pytest.mark.parametrize("dim", [5, 70])
def test_gradient_matrix_equal_to_error_is_the_plain_engine(gpu, dim, mode):
    n = 70
    err = spd_matrix(dim, dim)
    m = gpu.MODE_PER_CHAIN if mode == "per_chain" else gpu.MODE_POOLED
    with_g = gpu.HmcEngine(dim, n, likelihood=gpu.LIKE_QUADFORM, likelihood_params=err, seed=SEED, mode=m)
    plain = gpu.HmcEngine(dim, n, likelihood=gpu.LIKE_QUADFORM, likelihood_params=err, seed=SEED, mode=m)
    with_g.SetGradientMatrix(err)                       # before Start
    x0 = _start_points(dim, n)
    for e in (with_g, plain):
        e.Start(x0)
        if mode == "fixed":
            e.SetMeanEpsilon(-EPS); e.SetLeapFrog(LEAP)
    _same_engines(with_g, plain, "after Start")
    for k in range(2):
        with_g.Step(3); plain.Step(3)
        _same_engines(with_g, plain, f"block {k}")
    if mode == "pooled":
        assert with_g.tuning == plain.tuning
        assert np.array_equal(with_g.covariance, plain.covariance)
    with_g.SetGradientMatrix(None)                      # cleared: the plain path again, from the same state
    with_g.Step(3); plain.Step(3)
    _same_engines(with_g, plain, "after clearing")
    plain.SetGradientMatrix(err)                        # ... and set after Start
    with_g.Step(2); plain.Step(2)
    _same_engines(with_g, plain, "set after Start")
    assert plain.lane("naccept").sum() > 0


# ---- 8. a gradient matrix that is not Error -------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [5, 70])
def test_wrong_gradient_matrix_is_the_restated_reference_step(gpu, oracle, dim):
    n, steps = 3, 5
    err, grad = spd_matrix(dim, dim), spd_matrix(dim, 7 * dim + 1, spread=0.6)
    assert not np.array_equal(err, grad)
    e = gpu.HmcEngine(dim, n, likelihood=gpu.LIKE_QUADFORM, likelihood_params=err, seed=SEED)
    x0 = _start_points(dim, n)
    e.Start(x0)
    e.SetMeanEpsilon(-EPS); e.SetLeapFrog(LEAP)
    e.SetGradientMatrix(grad)
    e.Step(2); e.Step(steps - 2)
    q, m, logl = e.state()
    nacc, acceptance, proposed = e.lane("naccept"), e.lane("acceptance"), e.lane("logl_proposed")
    for c in range(n):
        r = HmcGradientRef(oracle, dim,
                           gradient=lambda p: oracle.hmc_gradient(oracle.LIKE_QUADFORM, p, params=grad),
                           potential=lambda p: oracle.hmc_potential(oracle.LIKE_QUADFORM, p, params=err,
                                                                    potential_from_gradient=True),
                           abs_epsilon=EPS, leapfrog=LEAP, seed=SEED, chain_id=c)
        r.start(x0[:, c])
        r.run(steps)
        assert np.array_equal(q[:, c], np.array(r.accepted)) and np.array_equal(m[:, c], np.array(r.momentum)), c
        assert logl[c] == -r.accepted_potential and proposed[c] == -r.proposed_potential
        assert nacc[c] == r.naccept and acceptance[c] == r.acceptance
    assert nacc.sum() > 0


# ---- 9. errors -------------------------------------------------------------------------------------------------------
def test_gradient_matrix_errors(gpu):
    dim = 5
    err = spd_matrix(dim, dim)
    iso = gpu.HmcEngine(dim, 8)
    with pytest.raises(gpu.SmcmcError) as ex:
        iso.SetGradientMatrix(err)
    assert ex.value.status == 1                                       # SMCMC_ERR_INVALID: not the quadratic form
    fused = gpu.HmcEngine(dim, 8, likelihood=gpu.LIKE_QUADFORM, likelihood_params=err, exact=False)
    with pytest.raises(gpu.SmcmcError) as ex:
        fused.SetGradientMatrix(err)
    assert ex.value.status == 5                                       # SMCMC_ERR_UNSUPPORTED: reference order only
    quad = gpu.HmcEngine(dim, 8, likelihood=gpu.LIKE_QUADFORM, likelihood_params=err)
    with pytest.raises(gpu.SmcmcError) as ex:
        quad.SetGradientMatrix(err[:2])                                # not dim*dim
    assert ex.value.status == 1
    quad.SetGradientMatrix(err)
    assert quad._lib.smcmc_hmc_set_exact_arithmetic(quad._h, 0) == 5   # ... whichever comes first


def test_a_user_library_without_a_gradient_still_refuses_type_0(gpu):
    if not os.path.exists(ASYM_LIB):
        gpu._build_mod.build(user_likelihood=ASYM_HEADER)
    e = gpu.HmcEngine(8, 64, likelihood=gpu.LIKE_USER, likelihood_params=np.array([-1.0, 100.0]), seed=5, library=ASYM_LIB)
    assert not e.has_gradient
    e.Start(np.full(8, 0.5))
    with pytest.raises(gpu.SmcmcError):
        e.Step(1, gradient_type=0)


# ---- 10. the reference's claim: a wrong gradient leaves the target distribution alone -------------------------------
def test_wrong_gradient_leaves_the_target_distribution_invariant(gpu):
    """Chains started from exact draws of N(0, C) and moved by 30 HMC steps whose gradient uses a BadGrad.C-style wrong
    matrix: the kernel leaves N(0, C) invariant whatever the gradient (TSimpleHMC.H:101-108), the chains are independent,
    so after the last step every coordinate is exactly N(0, C_ii): twelve checks at five standard errors."""
    cov, err, gerr = badgrad_matrices(STAT_DIM, STAT_SEED, STAT_MAX_CURVATURE)
    e = gpu.HmcEngine(STAT_DIM, STAT_CHAINS, likelihood=gpu.LIKE_QUADFORM, likelihood_params=err, seed=STAT_SEED)
    e.Start(stat_start_points(cov))
    e.SetMeanEpsilon(-STAT_EPS); e.SetLeapFrog(STAT_LEAP)
    e.SetGradientMatrix(gerr)
    e.Step(STAT_STEPS)
    q = e.state()[0]
    naccept = e.lane("naccept")
    print("accepted", naccept.sum(), "of", STAT_CHAINS * STAT_STEPS)
    assert stat_bounds_hold(q, cov)
    assert naccept.sum() > 0
