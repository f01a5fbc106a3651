"""The host side of the trace moments (smcmc.TraceMoments) and the restatements the GPU tests judge by
(tests/trace_moments_ref.py): nothing here launches a kernel."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("smcmc_trace_moments_ref",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "trace_moments_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def _sums(x, centre=None):
    """Raw sums of x[entries][dim] about a centre, plain numpy."""
    y = x - (0.0 if centre is None else np.asarray(centre)[None, :])
    return y.sum(axis=0), y.T @ y


def _ar1(entries, dim, seed, offset):
    rng = np.random.default_rng(seed)
    x = np.zeros((entries, dim))
    x[0] = rng.standard_normal(dim)
    for t in range(1, entries):
        x[t] = 0.9 * x[t - 1] + rng.standard_normal(dim)
    return x * np.linspace(0.5, 3.0, dim)[None, :] + np.asarray(offset)[None, :]


def test_trace_moments_class_equals_the_macro(smcmc):
    """TraceMoments on hand-made sums about the origin is MakeCovariance.C:63-89."""
    x = _ar1(600, 4, 1, [3.0, -40.0, 0.0, 1e3])
    macro = ref.make_covariance(x)
    m = smcmc.TraceMoments(macro["sum"], macro["sumsq"], 30, 20)
    assert m.n == 600.0
    assert np.array_equal(m.mean, macro["avg"])
    assert np.allclose(m.covariance, macro["covariance"], rtol=1e-13, atol=0)
    assert np.allclose(m.spread, macro["spread"], rtol=1e-12)
    # about a centre the covariance is the same covariance and the mean the same mean
    c = np.array([3.1, -39.0, 0.2, 990.0])
    about = smcmc.TraceMoments(*_sums(x, c), 30, 20, c)
    assert np.allclose(about.mean, macro["avg"], rtol=1e-13)
    assert np.allclose(about.covariance, np.cov(x.T, bias=True), rtol=1e-11)
    assert np.allclose(macro["covariance"], np.cov(x.T, bias=True), rtol=1e-6)     # what the origin costs at 1e3 +- 3


def test_spread_and_correlation(smcmc):
    rng = np.random.default_rng(5)
    z = rng.standard_normal((5000, 3))
    x = np.stack([2.0 * z[:, 0], z[:, 0] + z[:, 1], 0.1 * z[:, 2] + 7.0], axis=1)
    m = smcmc.TraceMoments(*_sums(x), 50, 100)
    cov = np.cov(x.T, bias=True)
    assert np.allclose(m.spread, x.std(axis=0), rtol=1e-10)
    assert np.allclose(m.correlation, np.corrcoef(x.T), rtol=1e-9, atol=1e-12)
    assert np.allclose(np.diag(m.correlation), 1.0, rtol=1e-12)
    assert np.allclose(m.covariance, cov, rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError):
        smcmc.TraceMoments(np.zeros(3), np.zeros((2, 2)), 1, 1)


def test_halves_with_different_centres_add_to_the_whole(smcmc):
    x = _ar1(800, 5, 2, [0.0, 10.0, -3.0, 100.0, 1.0]).reshape(40, 20, 5)        # [slot][chain][dim]
    whole = smcmc.TraceMoments(*_sums(x.reshape(-1, 5)), 40, 20)
    c1, c2 = x[:, :8].mean(axis=(0, 1)), x[:, 8:].mean(axis=(0, 1)) + 0.5
    a = smcmc.TraceMoments(*_sums(x[:, :8].reshape(-1, 5), c1), 40, 8, c1)
    b = smcmc.TraceMoments(*_sums(x[:, 8:].reshape(-1, 5), c2), 40, 12, c2)
    both = a + b
    assert both.nchains == 20 and both.n == whole.n and np.array_equal(both.centre, c1)
    assert np.allclose(both.mean, whole.mean, rtol=1e-12)
    assert np.allclose(both.covariance, whole.covariance, rtol=1e-12, atol=1e-12)
    back = both.about(np.zeros(5))
    assert np.allclose(back.sum, whole.sum, rtol=1e-12) and np.allclose(back.sumsq, whole.sumsq, rtol=1e-12)
    with pytest.raises(ValueError):
        a + smcmc.TraceMoments(*_sums(x[:20, 8:].reshape(-1, 5)), 20, 12)


def test_exact_sums_are_exact():
    """The limb arithmetic of exact_sums against Python integers, far centre included."""
    x = _ar1(70, 3, 3, [3.0, -40.0, 1e-3])
    for centre in (None, x.mean(axis=0), x.mean(axis=0) + 1e8):
        total, gram, a_total, a_gram = ref.exact_sums(x, centre)
        c = [Fraction(0)] * 3 if centre is None else [Fraction(*float(v).as_integer_ratio()) for v in centre]
        Y = [[Fraction(*float(v).as_integer_ratio()) - c[d] for d, v in enumerate(row)] for row in x]
        for i in range(3):
            assert total[i] == sum(r[i] for r in Y)
            assert a_total[i] <= float(sum(abs(r[i]) for r in Y)) and a_total[i] >= 0.999999 * float(sum(abs(r[i]) for r in Y))
            for j in range(3):
                assert gram[i, j] == sum(r[i] * r[j] for r in Y)
                s = float(sum(abs(r[i] * r[j]) for r in Y))
                assert 0.999999 * s <= a_gram[i, j] <= s
    # the macro restatement is itself within the bound it is used with
    macro = ref.make_covariance(x)
    assert ref.check_rounding_bound(macro["sum"], macro["sumsq"], x, None) <= 1.0


def test_reference_draws_are_a_chain_steps(oracle):
    """The Cholesky chain's layout of the normals, on stream 0, is oracle.step_draws."""
    for dim in (1, 2, 5, 8, 50, 65):
        for chain, step in ((0, 0), (7, 3), (129, 100000)):
            want, _ = oracle.step_draws(9, chain, step, dim)
            assert np.array_equal(ref.entry_normals(oracle, 9, chain, step, dim, stream=0), want)
    assert not np.array_equal(ref.entry_normals(oracle, 9, 7, 3, 8), oracle.step_draws(9, 7, 3, 8)[0])   # its own stream


def test_reference_cholesky_chain_round_trip(oracle, smcmc):
    """The reference chain, through the macro restatement, passes the statistical assertion of the GPU round trip."""
    dim, nslots, nchains = 8, 64, 256
    sigma = ref.random_spd(dim, 11, 0.1, 10.0)
    mean = np.linspace(-5.0, 50.0, dim)
    trace, U = ref.cholesky_chain(oracle, mean, sigma, nslots, nchains, seed=20240607)
    assert np.allclose(U.T @ U, sigma, rtol=1e-12) and np.array_equal(U, np.triu(U))
    macro = ref.make_covariance(ref.entries_of(trace) - mean[None, :])
    m = smcmc.TraceMoments(macro["sum"], macro["sumsq"], nslots, nchains, mean)
    ref.gaussian_round_trip(m.mean, m.covariance, mean, sigma, nslots * nchains)
    # the assertion has teeth: a chain of the wrong covariance fails it
    with pytest.raises(AssertionError):
        ref.gaussian_round_trip(m.mean, m.covariance, mean, 1.2 * sigma, nslots * nchains)
    with pytest.raises(AssertionError):
        ref.gaussian_round_trip(m.mean, m.covariance, mean + 0.2 * np.sqrt(np.diag(sigma)), sigma, nslots * nchains)
    # a slice of the chains is a chain_offset
    part, _ = ref.cholesky_chain(oracle, mean, sigma, 2, 3, seed=20240607, chain_offset=5)
    assert np.array_equal(part, trace[:2, :, 5:8])
    assert ref.cholesky_chain(oracle, mean, -sigma, 1, 1, seed=1) == (None, None)


def test_cholesky_chain_needs_a_device(smcmc):
    """Without a device the fill fails loudly: there is no host version behind it."""
    import torch
    if torch.cuda.is_available():
        return                           # tests/test_gpu_trace_moments.py has the device's side
    with pytest.raises(smcmc.SmcmcError) as err:
        smcmc.cholesky_chain(np.zeros(2), np.eye(2), 1, 1)
    assert err.value.status == 7
