"""The host side of the convergence reducer (smcmc.Convergence: split R-hat, Geyer's tau, the multi-chain ESS) against
the restatement in tests/convergence_ref.py, fed with the restatement's sums: nothing here launches a kernel."""
import importlib.util
import os
import warnings

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("smcmc_convergence_ref",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "convergence_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def _ar1(nslots, dim, nchains, seed, phi=0.9, spread=0.0):
    """x[slot][dim][chain]: stationary AR(1) of unit innovation, every chain about a level of its own (`spread`)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((nslots, dim, nchains))
    x[0] = rng.standard_normal((dim, nchains)) / np.sqrt(1.0 - phi * phi)
    for t in range(1, nslots):
        x[t] = phi * x[t - 1] + rng.standard_normal((dim, nchains))
    return x + spread * rng.standard_normal((1, dim, nchains))


def _of(smcmc, x, S=2, centre=None):
    """(Convergence fed with the restatement's sums, the restatement's sums)."""
    r = ref.sums(x, S, centre)
    return smcmc.Convergence(r["sum"], r["sumsq_of_sums"], r["within"], r["L"], r["M"], centre), r


def _close(a, b, what):
    assert np.allclose(a, b, rtol=1e-12, atol=0.0, equal_nan=True), (what, a, b)


# (nslots, nchains, dim, S): L = 20 < 64;  M = 2 (one chain in halves);  L = 43 with r = 2 leading slots dropped
@pytest.mark.parametrize("nslots,nchains,dim,S", [(40, 6, 3, 2), (300, 1, 2, 2), (131, 5, 2, 3)])
def test_class_equals_the_restatement(smcmc, nslots, nchains, dim, S):
    x = _ar1(nslots, dim, nchains, nslots + nchains, phi=0.6, spread=0.5) + np.linspace(3.0, -40.0, dim)[None, :, None]
    centre = x.mean(axis=(0, 2)) + 0.25
    c, r = _of(smcmc, x, S, centre)
    want = ref.statistics(r["sum"], r["sumsq_of_sums"], r["within"], r["L"], r["M"])
    assert (c.L, c.M) == ref.layout(nslots, S)[:1] + (S * nchains,)
    assert c.rho().shape == (min(64, c.L), dim)
    for name in ("W", "var_of_means", "var_plus"):
        _close(getattr(c, name), want[name], name)
    for name in ("rhat", "rho", "tau", "ess"):
        _close(getattr(c, name)(), want[name], name)
    assert np.array_equal(c.truncated(), want["truncated"])
    assert np.all(np.isfinite(c.rhat())) and np.all(c.rhat() > 1.0)          # the chains sit at different levels
    # the pooled mean does not depend on the centre
    _close(c.mean(), x[ref.layout(nslots, S)[1]:].mean(axis=(0, 2)), "mean")


def _iid(seed):
    return np.random.default_rng(seed).standard_normal((500, 1, 128))


def test_independent_normal_draws(smcmc):
    """128 chains x 500 slots of independent N(0, 1), halves: R-hat is 1 and tau is 1.  A numpy prototype of the
    restatement over the seeds 0-9 gave |rhat - 1| <= 3e-4 and tau in 0.966 .. 0.997; this is seed 0."""
    c, _ = _of(smcmc, _iid(0))
    print("rhat %.6f tau %.4f" % (c.rhat()[0], c.tau()[0]))
    assert abs(c.rhat()[0] - 1.0) < 0.01
    assert 0.9 < c.tau()[0] < 1.1
    assert abs(c.ess()[0] / (256 * 250.0) - 1.0 / c.tau()[0]) < 1e-12


def test_shifted_chains_are_seen(smcmc):
    """The same draws with every second chain shifted by delta = 2 sigma: var+ / W = 1 + delta^2 / 4, R-hat = 1.414
    (the prototype gave 1.410 .. 1.421 over the seeds 0-9).  The pooled reducers cannot tell this from a wide target."""
    x = _iid(0)
    x[:, :, 1::2] += 2.0
    c, _ = _of(smcmc, x)
    print("rhat %.4f" % c.rhat()[0])
    assert c.rhat()[0] > 1.3


def test_ar1_autocorrelation_time(smcmc):
    """Stationary AR(1), phi = 0.9, 256 chains x 2 000 slots, halves: tau = (1 + phi) / (1 - phi) = 19.  A numpy
    prototype of the restatement over the seeds 0-9 gave 18.56 .. 19.35; the margin of 10 % is about seven times that
    spread.  This is seed 0.  truncated() is seed-dependent here (True on eight of the ten seeds) and not asserted."""
    c, _ = _of(smcmc, _ar1(2000, 1, 256, 0))
    print("tau %.3f truncated %s rhat %.5f" % (c.tau()[0], c.truncated()[0], c.rhat()[0]))
    assert abs(c.tau()[0] - 19.0) <= 1.9


def test_a_constant_dimension_gives_nan_quietly(smcmc):
    x = _ar1(60, 2, 4, 3)
    x[:, 1, :] = 7.0
    c, _ = _of(smcmc, x, 2, np.array([0.0, 7.0]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rhat, tau, ess, rho, trunc = c.rhat(), c.tau(), c.ess(), c.rho(), c.truncated()
    assert np.isfinite(rhat[0]) and np.isnan(rhat[1])
    assert np.isfinite(tau[0]) and np.isnan(tau[1]) and np.isnan(ess[1]) and np.all(np.isnan(rho[:, 1]))
    assert trunc.shape == (2,)
    # one segment-chain has no variance of the means: M < 2
    single, _ = _of(smcmc, x[:, :, :1], 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.all(np.isnan(single.rhat()))


def test_ranks_add(smcmc):
    x = _ar1(90, 3, 10, 5, spread=0.3)
    centre = np.array([0.1, -0.2, 0.3])
    whole, _ = _of(smcmc, x, 2, centre)
    a, _ = _of(smcmc, x[:, :, :4], 2, centre)
    b, _ = _of(smcmc, x[:, :, 4:], 2, centre)
    both = a + b
    assert (both.L, both.M) == (whole.L, whole.M)
    for name in ("sum", "sumsq_of_sums", "within"):
        _close(getattr(both, name), getattr(whole, name), name)
    for name in ("rhat", "tau", "ess", "mean"):
        assert np.allclose(getattr(both, name)(), getattr(whole, name)(), rtol=1e-12, atol=0.0), name


def test_adding_needs_the_same_segments_and_centre(smcmc):
    x = _ar1(90, 2, 4, 6)
    a, _ = _of(smcmc, x)
    with pytest.raises(ValueError):
        a + _of(smcmc, x[:80])[0]                     # L = 40 against 45
    with pytest.raises(ValueError):
        a + _of(smcmc, x, 2, np.array([1.0, 0.0]))[0]
    with pytest.raises(ValueError):
        smcmc.Convergence(np.zeros(3), np.zeros(2), np.zeros((64, 3)), 10, 4)
