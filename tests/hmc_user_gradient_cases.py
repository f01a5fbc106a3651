"""What the tests of HMC with the caller's own gradient share: the example libraries, seeded matrices and the
statistical case of BadGrad.C (used by tests/test_gpu_hmc_user_gradient.py and tools/hmc_bad_gradient_cpu_check.py)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_LIB = os.path.join(ROOT, "root-simple-mcmc_amd", "lib", "libsmcmc_amd_user_grad.so")
GRAD_HEADER = os.path.join(ROOT, "examples", "user_likelihood_quadgrad.hip.h")
ASYM_LIB = os.path.join(ROOT, "root-simple-mcmc_amd", "lib", "libsmcmc_amd_user.so")
ASYM_HEADER = os.path.join(ROOT, "examples", "user_likelihood_asym.hip.h")


def spd_matrix(dim, seed, spread=0.3):
    """A seeded, exactly symmetric, well-conditioned SPD matrix: I + spread * (A A^T) / dim, condition number < 1 + 4 spread."""
    a = np.random.default_rng(seed).normal(size=(dim, dim))
    m = np.eye(dim) + spread * (a @ a.T) / dim
    return (m + m.T) / 2.0


def grad_lib(smcmc):
    """The example library with a gradient: built by __graft_entry__.build(); rebuilt here only if it is missing."""
    if not os.path.exists(GRAD_LIB):
        smcmc._build_mod.build(user_likelihood=GRAD_HEADER, output_name="user_grad")
    return GRAD_LIB


def badgrad_matrices(dim, seed, max_curvature=None):
    """BadGrad.C:43-150 in numpy: (Covariance, Error, GradientError).  Unit variances and 0.9 (j - i) / (dim - 1) on the
    anti-diagonal; the gradient's covariance has every variance scaled by N(1, 0.1) (at least 0.3) and every covariance
    moved by N(0, 0.3); both are shrunk towards the diagonal by 0.9 until positive definite.  BadGrad.C stops there; a
    gradient covariance that is only just positive definite has an inverse with a huge eigenvalue, on which a leapfrog
    of fixed step length diverges and every proposal is rejected (still correct, but nothing moves).  With
    max_curvature the perturbation is drawn again, from the same generator, until the largest eigenvalue of
    GradientError is below it."""
    def repair(c):
        while np.linalg.eigvalsh(c).min() <= 0.0:
            d = np.diag(np.diag(c))
            c = d + 0.9 * (c - d)
        return c
    cov = np.eye(dim)
    for i in range(dim):
        j = dim - 1 - i
        if j > i:
            cov[i, j] = cov[j, i] = 0.9 * (j - i) / (dim - 1.0)
    cov = repair(cov)
    rng = np.random.default_rng(seed)
    sym = lambda a: (a + a.T) / 2.0   # noqa: E731
    while True:
        gcov = cov.copy()
        for i in range(dim):
            for j in range(i, dim):
                if i == j:
                    s = rng.normal(1.0, 0.1)
                    while s < 0.3:
                        s = rng.normal(1.0, 0.1)
                    gcov[i, i] = cov[i, i] * s
                else:
                    gcov[i, j] = gcov[j, i] = cov[i, j] + rng.normal(0.0, 0.3)
        gerr = sym(np.linalg.inv(repair(gcov)))
        if max_curvature is None or np.linalg.eigvalsh(gerr).max() < max_curvature:
            break
    return cov, sym(np.linalg.inv(cov)), gerr


STAT_DIM, STAT_CHAINS, STAT_STEPS, STAT_SEED = 6, 8192, 30, 2024
# A leapfrog of step e on curvature k is stable for e^2 k < 4.  The stiffest direction of Covariance has variance 0.1
# (k = 10): a step of 0.15 gives 0.23.  The wrong gradient is kept to e^2 k < 1 (k < 44), so that trajectories move and
# some are accepted; how wrong it may be otherwise is BadGrad.C's.
STAT_EPS, STAT_LEAP = 0.15, 4
STAT_MAX_CURVATURE = 1.0 / (STAT_EPS * STAT_EPS)


def stat_start_points(cov, n=STAT_CHAINS):
    """exact draws of N(0, cov), one per chain: [dim][chain]"""
    z = np.random.default_rng(STAT_SEED + 1).standard_normal((cov.shape[0], n))
    return np.linalg.cholesky(cov) @ z


def stat_bounds_hold(q, cov):
    """every coordinate's mean within 5 sqrt(C_ii / n) and variance within 5 C_ii sqrt(2 / (n - 1)); prints the figures"""
    n = q.shape[1]
    ok = True
    for i in range(q.shape[0]):
        mean, var = q[i].mean(), q[i].var(ddof=1)
        bm, bv = 5.0 * np.sqrt(cov[i, i] / n), 5.0 * cov[i, i] * np.sqrt(2.0 / (n - 1))
        print(f"coordinate {i}: mean {mean:+.5f} (bound {bm:.5f})  variance {var:.5f} - {cov[i, i]:.5f} = "
              f"{var - cov[i, i]:+.5f} (bound {bv:.5f})")
        ok = ok and abs(mean) <= bm and abs(var - cov[i, i]) <= bv
    return ok
