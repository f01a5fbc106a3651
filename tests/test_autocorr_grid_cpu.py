"""The host side of the lag-grid autocorrelation (autocorrelation_plan, MacroAutocorrelation, AutocorrelationGrid)
against the literal restatement of MakeAutocorrelation.C in tests/autocorr_grid_ref.py.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_autocorr_grid_ref", os.path.join(HERE, "autocorr_grid_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


# entries: (maxLag, bins, lagStep, trials, number of lags)
PLANS = {100: (90, 90, 1, 100, 89), 300: (282, 100, 1, 300, 281), 399: (379, 100, 1, 399, 378),
         400: (380, 100, 1, 400, 379), 4000: (3936, 100, 19, 4000, 208), 40000: (30000, 100, 150, 40000, 200)}


@pytest.mark.parametrize("entries", sorted(PLANS))
def test_plan_constants(smcmc, entries):
    p = smcmc.autocorrelation_plan(entries)
    assert (p.max_lag, p.bins, p.lag_step, p.trials, len(p.lags)) == PLANS[entries]
    ref = R.plan(entries)
    assert (ref["maxLag"], ref["bins"], ref["lagStep"], ref["trials"], len(ref["lags"])) == PLANS[entries]
    assert list(p.lags) == ref["lags"] == list(range(1, p.max_lag, p.lag_step))
    assert list(p.lag_bins) == [int(p.bins * (lag + 0.5) / p.max_lag) for lag in ref["lags"]]
    assert p.lag_bins.min() >= 0 and p.lag_bins.max() < p.bins
    assert np.allclose(p.bin_centres, (np.arange(p.bins) + 0.5) * p.max_lag / p.bins, rtol=1e-15)


def test_plan_never_asks_for_more_lags_than_one_call_takes(smcmc):
    """398 lags are the most of any number of entries (420 entries: maxLag = 399, the last with lagStep = 1; 421 give
    maxLag = 400 and lagStep = 2): below SMCMC_AUTOCORR_GRID_MAX_LAGS.  418 entries give maxLag = 397 and 396 lags."""
    counts = {n: len(smcmc.autocorrelation_plan(n).lags) for n in range(4, 3000)}
    assert max(counts.values()) == 398 == counts[420] and counts[421] == 200 and counts[418] == 396
    p = smcmc.autocorrelation_plan(420)
    assert (p.max_lag, p.bins, p.lag_step, p.trials) == (399, 100, 1, 420)
    assert len(smcmc.autocorrelation_plan(30000 * 4).lags) <= 398
    assert smcmc._capi.AUTOCORR_GRID_MAX_LAGS == 512 >= 398
    with pytest.raises(ValueError):
        smcmc.autocorrelation_plan(3)


def _ar1(n, dim=1, seed=1, phi=0.8, offset=3.0):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, dim))
    for t in range(1, n):
        s[t] = phi * s[t - 1] + rng.standard_normal(dim)
    return s + offset


def _numpy_sums(x, p):
    """x[slot][dim][chain] -> (sum, sumsq, lagged) in doubles over the last p.trials slots on p.lags."""
    x = x[x.shape[0] - p.trials:]
    n = x.shape[0]
    lagged = np.array([(x[k:] * x[:n - k]).sum(axis=(0, 2)) for k in p.lags])
    return x.sum(axis=(0, 2)), (x * x).sum(axis=(0, 2)), lagged


@pytest.mark.parametrize("n", [100, 1000, 4000])
def test_from_sums_reproduces_the_macro_on_one_chain(smcmc, n):
    """One chain of an AR(1) series (phi = 0.8 about 3.0): the binned pooled-sum form equals the macro's ring-buffer
    loop.  At n = 100 no lag falls into bin 0 (lag 1 sits at 1.5 of a bin width 1): NaN on both sides."""
    s = _ar1(n)
    p = smcmc.autocorrelation_plan(n)
    m = smcmc.MacroAutocorrelation.from_sums(p, *_numpy_sums(s[:, :, None], p), 1)
    ref = R.macro_loop(s)
    assert m.autocorr.shape == ref["autocorr"].shape == (1, p.bins)
    empty = np.isnan(ref["autocorr"][0])
    assert np.array_equal(np.isnan(m.autocorr[0]), empty)
    assert bool(empty[0]) == (n == 100) and empty.sum() == (1 if n == 100 else 0)
    assert np.allclose(m.autocorr[:, ~empty], ref["autocorr"][:, ~empty], rtol=0, atol=1e-12)
    print("n=%d: max |autocorr - macro| = %.3g" % (n, np.max(np.abs(m.autocorr[:, ~empty] - ref["autocorr"][:, ~empty]))))
    assert np.allclose(m.mean, ref["mean"], rtol=1e-14) and np.allclose(m.err2, ref["err2"], rtol=1e-11)
    assert np.allclose(m.bin_centres, ref["bin_centres"], rtol=1e-15)
    if n > 100:                                                       # AR(1): a(k) = phi^k at the first bins' lags
        first = [k for k, b in zip(p.lags, p.lag_bins) if b == 0]
        assert abs(m.autocorr[0, 0] - np.mean(0.8 ** np.array(first))) < 0.1


def test_ranks_add_their_sums(smcmc):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((300, 3, 40)).cumsum(axis=0) * 0.01 + rng.standard_normal((300, 3, 40))
    p = smcmc.autocorrelation_plan(300)
    whole = smcmc.MacroAutocorrelation.from_sums(p, *_numpy_sums(x, p), 40)
    halves = (smcmc.MacroAutocorrelation.from_sums(p, *_numpy_sums(x[:, :, :20], p), 20)
              + smcmc.MacroAutocorrelation.from_sums(p, *_numpy_sums(x[:, :, 20:], p), 20))
    assert halves.nchains == 40
    assert np.allclose(halves.autocorr, whole.autocorr, rtol=1e-12, atol=0)
    assert np.allclose(halves.mean, whole.mean, rtol=1e-12) and np.allclose(halves.err2, whole.err2, rtol=1e-12)
    with pytest.raises(ValueError):
        whole + smcmc.MacroAutocorrelation.from_sums(smcmc.autocorrelation_plan(301), *_numpy_sums(x, p)[:2],
                                                     np.zeros((len(smcmc.autocorrelation_plan(301).lags), 3)), 40)
    # the grid sums themselves
    lags = np.arange(1, 41) * 3 + 2
    def grid(y):
        lagged = np.array([(y[k:] * y[:300 - k]).sum(axis=(0, 2)) for k in lags])
        return smcmc.AutocorrelationGrid(lags, y.sum(axis=(0, 2)), (y * y).sum(axis=(0, 2)), lagged, 300, y.shape[2])
    g, h = grid(x), grid(x[:, :, :20]) + grid(x[:, :, 20:])
    assert np.array_equal(g.counts, (300 - lags) * 40.0) and np.array_equal(h.counts, g.counts)
    assert np.allclose(h.rho(), g.rho(), rtol=1e-12, atol=1e-14)
    mean = x.mean(axis=(0, 2))
    want = np.array([(x[k:] * x[:300 - k]).mean(axis=(0, 2)) - mean * mean for k in lags]) / x.var(axis=(0, 2))
    assert np.allclose(g.rho(), want, rtol=1e-10, atol=1e-12)
    with pytest.raises(ValueError):
        g + smcmc.AutocorrelationGrid(lags + 1, g.sum, g.sumsq, g.lagged, 300, 40)


def test_average_and_spread_over_the_dimensions(smcmc):
    s = _ar1(1000, dim=3, seed=5) * np.array([1.0, 2.5, 0.3])
    p = smcmc.autocorrelation_plan(1000)
    m = smcmc.MacroAutocorrelation.from_sums(p, *_numpy_sums(s[:, :, None], p), 1)
    assert m.autocorr.shape == (3, p.bins)
    assert np.array_equal(m.average, np.mean(m.autocorr, axis=0))
    assert np.array_equal(m.spread, np.std(m.autocorr, axis=0))
    ref = R.macro_loop(s)                                              # the profile the macro fills, option "S"
    assert np.allclose(m.average, ref["average"], rtol=0, atol=1e-12)
    assert np.allclose(m.spread, ref["spread"], rtol=0, atol=1e-9)     # sqrt(<a^2> - <a>^2) there: it cancels
    # a reference point enters through the edges of the lagged sums only: O(lag / trials)
    c = np.array([2.5, 8.0, 1.0])
    shifted = smcmc.MacroAutocorrelation.from_sums(p, *_numpy_sums(s[:, :, None] - c[None, :, None], p), 1, centre=c)
    assert np.allclose(shifted.mean, m.mean, rtol=1e-13) and np.allclose(shifted.err2, m.err2, rtol=1e-9)
    near = p.bin_centres < 100
    assert np.max(np.abs(shifted.autocorr[:, near] - m.autocorr[:, near])) < 100 / 1000 * 3


def test_binding_declares_the_symbol(smcmc):
    import ctypes as C
    res, args = smcmc.SIGNATURES["smcmc_autocorrelation_grid_sums"]
    assert res is C.c_int and len(args) == 14
    assert args[7:10] == [C.c_int, C.c_int, C.c_int]
    for cls in (smcmc.Engine, smcmc.HmcEngine, smcmc.VaatEngine):
        assert callable(cls.AutocorrelationGrid) and callable(cls.MakeAutocorrelation)
