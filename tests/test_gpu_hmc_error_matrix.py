"""UpdateErrorMatrix's eigenvalue step (TSimpleHMC.H:760-830) of the per-chain HMC mode: the device routine against the
pooled mode's host routine (HmcShared), bit for bit, through smcmc_selftest_hmc_error_matrix.  Chain-level runs rarely
reach the repair loop (:766-809); this does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _spd(dim, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((dim, dim)) / np.sqrt(dim)
    return a @ a.T + 0.1 * np.eye(dim)


def _indefinite(dim, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((dim, dim))
    return 0.5 * (a + a.T)


def _repeated(dim, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((dim, dim)))
    ev = np.repeat([2.0, 0.5], [dim - dim // 2, dim // 2])
    return (q * ev) @ q.T


def _zero_row(dim, seed):
    c = _spd(dim, seed)
    k = dim // 2
    c[k, :] = 0.0
    c[:, k] = 0.0
    return c


def _same(gpu, cov, est_trace):
    dev = gpu.selftest_hmc_error_matrix(cov, est_trace, device=0)
    host = gpu.selftest_hmc_error_matrix(cov, est_trace, device=-1)
    assert np.array_equal(dev[0], host[0]), "repaired covariance"
    assert np.array_equal(dev[1], host[1]), "eigenvalues"
    assert dev[2] == host[2], (dev[2], host[2])
    return host


@pytest.mark.parametrize("dim", [2, 5, 63, 64, 200, 512])
def test_error_matrix_spd(gpu, dim):
    cov = _spd(dim, dim)
    _, eig, t = _same(gpu, cov, float(dim))
    assert t["passes"] == 0
    assert np.allclose(np.sort(eig), np.linalg.eigvalsh(cov), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("dim", [2, 5, 63, 64, 200])
def test_error_matrix_repair_loop(gpu, dim):
    cov = _indefinite(dim, dim + 1)
    rep, eig, t = _same(gpu, cov, float(np.abs(np.diag(cov)).sum()))
    assert t["passes"] >= 1 and np.all(eig >= 0)
    assert np.array_equal(rep, np.diag(np.diag(rep)))


@pytest.mark.parametrize("dim", [5, 64, 130])
def test_error_matrix_special_matrices(gpu, dim):
    _same(gpu, _repeated(dim, 1), float(dim))
    _same(gpu, _zero_row(dim, 2), float(dim))
    _same(gpu, np.diag(np.linspace(0.5, 3.0, dim)), float(dim))
    neg = np.diag(np.linspace(-1.0, 3.0, dim))
    assert _same(gpu, neg, 0.0)[2]["passes"] >= 1                # r = 0: the negative diagonal becomes zero
