"""Restatement of MakeAutocorrelation.C in our own words (test helper, imported by the test modules; it shares no code
with the kernels or with engine.py), and the exact sums and the rounding bound the device reducer
smcmc_autocorrelation_grid_sums is judged against.

  plan                 the macro's constants from the number of entries (:62, 70-73, 98-99, 104-106)
  macro_loop           the macro's loop, literally, in doubles: ring buffer, `fills <= lag` break, per-bin fills,
                       the Pearson form per bin, the profile over the dimensions
  grid_lags            lag_first + i lag_step
  integer_grid_sums    sum, sumsq, lagged of integer data, in int64
  exact_grid_sums      the same of doubles in exact rational arithmetic, with the sums of absolute values
  check_rounding_bound |device - exact| against the bound below

The macro holds its ring buffer and its histograms in floats; the restatement holds doubles (the deviation
include/smcmc.h states), so it is the macro's arithmetic with the single-precision roundings taken out.

The rounding bound, as tests/test_autocorrelation.py derives it.  u = 2^-53, gamma_m = m u / (1 - m u); y = x - centre is
one rounding per factor, the fused multiply-add rounds once per term, the butterfly and the block sum are additions of
the same sum: a row of n terms is within 2 gamma_(n+2) sum |y_t y_(t-k)| of the exact sum of the exact products (the
factor 2 for the second order, as tests/truth.py has it), sumsq likewise with k = 0, and the plain sum within
2 gamma_(n+1) sum |y|.  The sums of absolute values that scale a bound are taken in doubles and rounded DOWN by 2^-20
relative: an underestimate keeps the bound honest.
"""
import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
DOWN = 1.0 - 2.0 ** -20


def gamma(m):
    return m * U / (1 - m * U)


def F(v):
    return Fraction(*float(v).as_integer_ratio())


# ---- the macro ---------------------------------------------------------------------------------------------------------

def plan(entries, depth=30000, nbins=100, precision=0.01):
    """dict(entries, depth, maxLag, bins, lagStep, trials, lags): MakeAutocorrelation.C:62, 70-73, 98-99, 104-106, 117."""
    maxLag = int(entries - math.sqrt(entries))                       # :71, a double truncated into an int
    maxLag = min(maxLag, depth)                                      # :72
    bins = min(nbins, maxLag)                                        # :73
    lagStep = int(0.5 * maxLag / bins)                               # :98
    if lagStep < 1:                                                  # :99
        lagStep = 1
    trials = int(maxLag + 1.0 / (precision * precision * precision))  # :105
    trials = min(trials, entries)                                    # :106
    lags = []
    lag = 1
    while lag < maxLag:                                              # :117
        lags.append(lag)
        lag += lagStep
    return dict(entries=entries, depth=depth, maxLag=maxLag, bins=bins, lagStep=lagStep, trials=trials, lags=lags)


def _find_bin(x, nbins, lo, hi):
    """The fixed-width axis of include/smcmc.h, 0-based; None outside [lo, hi)."""
    if x < lo or not (x < hi):
        return None
    return int(nbins * (x - lo) / (hi - lo))


def macro_loop(accepted, depth=30000):
    """accepted[entry][dim] (one chain): the macro from :62 to :148 with doubles where it has floats.  Returns
    dict(bin_centres[bin], mean[dim], err2[dim], autocorr[dim][bin], average[bin], spread[bin], counts[bin])."""
    accepted = np.asarray(accepted, dtype=np.float64)
    entries, dim = accepted.shape
    p = plan(entries, depth)
    maxLag, bins, lagStep, trials = p["maxLag"], p["bins"], p["lagStep"], p["trials"]
    ring = [[0.0] * depth for _ in range(dim)]                       # :63
    nextBuffer = -1
    mean_n, mean_s, mean_s2 = [0] * dim, [0.0] * dim, [0.0] * dim    # meanValues, a profile: entries, sum, sum of squares
    corr = [[0.0] * bins for _ in range(dim)]                        # autoCorr[i].first
    count = [[0.0] * bins for _ in range(dim)]                       # autoCorr[i].second
    lag_bin = {lag: _find_bin(lag + 0.5, bins, 0.0, float(maxLag)) for lag in p["lags"]}
    fills = 0
    for entry in range(entries - trials, entries):                   # :108
        nextBuffer = (nextBuffer + 1) % depth                        # :110
        fills += 1
        for i in range(dim):
            val = float(accepted[entry, i])
            mean_n[i] += 1                                           # :115
            mean_s[i] += val
            mean_s2[i] += val * val
            buf = ring[i]
            buf[nextBuffer] = val                                    # :116
            hist, cnt = corr[i], count[i]
            lag = 1
            while lag < maxLag:                                      # :117
                if fills <= lag:                                     # :118
                    break
                lVal = buf[(nextBuffer + depth - lag) % depth]       # :119-120
                b = lag_bin[lag]
                hist[b] += lVal * val                                # :121
                cnt[b] += 1.0                                        # :122
                lag += lagStep
    nan = float("nan")
    autocorr = np.zeros((dim, bins))
    means, err2 = np.zeros(dim), np.zeros(dim)
    prof_n, prof_s, prof_s2 = [0] * bins, [0.0] * bins, [0.0] * bins  # avgCorr
    for i in range(dim):
        mean = mean_s[i] / mean_n[i]                                 # :132
        e2 = mean_s2[i] / mean_n[i] - mean * mean                    # :133, option "s": the spread, here squared
        means[i], err2[i] = mean, e2
        for j in range(bins):
            v, e = corr[i][j], count[i][j]                           # :136, 138
            a = (v / e - mean * mean) / e2 if e != 0.0 else nan      # :139 (0/0 in C)
            autocorr[i, j] = a
            prof_n[j] += 1                                           # :146
            prof_s[j] += a
            prof_s2[j] += a * a
    average = np.array([prof_s[j] / prof_n[j] for j in range(bins)])
    spread = np.array([math.sqrt(max(prof_s2[j] / prof_n[j] - (prof_s[j] / prof_n[j]) ** 2, 0.0))
                       if prof_s[j] == prof_s[j] else nan for j in range(bins)])
    centres = np.array([(j + 0.5) * maxLag / bins for j in range(bins)])
    return dict(bin_centres=centres, mean=means, err2=err2, autocorr=autocorr, average=average, spread=spread,
                counts=np.array(count[0]))


# ---- the grid sums -----------------------------------------------------------------------------------------------------

def grid_lags(lag_first, lag_step, nlags):
    return [lag_first + i * lag_step for i in range(nlags)]


def integer_grid_sums(y, lags):
    """y[slot][dim][chain], an int64 array of integers small enough that nothing here leaves int64 (the caller says why):
    (sum[dim], sumsq[dim], lagged[lag][dim]) exactly."""
    assert y.dtype == np.int64
    nslots = y.shape[0]
    lagged = np.zeros((len(lags), y.shape[1]), dtype=np.int64)
    for i, k in enumerate(lags):
        if k < nslots:
            lagged[i] = (y[k:] * y[:nslots - k]).sum(axis=(0, 2))
    return y.sum(axis=(0, 2)), (y * y).sum(axis=(0, 2)), lagged


def _dyadic(a, extra):
    """Doubles as Python ints over one power of two: (object array of a's shape, object array of `extra`, den)."""
    flat = [float(v).as_integer_ratio() for v in np.ravel(a)] + [float(v).as_integer_ratio() for v in extra]
    den = max(d for _, d in flat)
    ints = np.empty(len(flat), dtype=object)
    ints[:] = [n * (den // d) for n, d in flat]
    return ints[:np.size(a)].reshape(np.shape(a)), ints[np.size(a):], den


def _isum(a):
    return sum(np.asarray(a, dtype=object).ravel().tolist(), 0)


def exact_grid_sums(x, centre, lags):
    """x[slot][dim][chain] doubles, centre[dim] or None: dict(sum[dim], sumsq[dim], lagged[lag][dim]) as Fractions of
    y = x - centre taken exactly, and abs_sum[dim], abs_sumsq[dim], abs_lagged[lag][dim]: the sums of |y|, y^2 and
    |y_t y_(t-k)| in doubles, rounded down."""
    x = np.asarray(x, dtype=np.float64)
    nslots, dim, _ = x.shape
    c = np.zeros(dim) if centre is None else np.asarray(centre, dtype=np.float64)
    X, C, den = _dyadic(x, c)
    Y = X - C[None, :, None]
    a = np.abs(x - c[None, :, None])
    out = dict(sum=np.empty(dim, dtype=object), sumsq=np.empty(dim, dtype=object),
               lagged=np.empty((len(lags), dim), dtype=object), abs_sum=a.sum(axis=(0, 2)) * DOWN,
               abs_sumsq=(a * a).sum(axis=(0, 2)) * DOWN, abs_lagged=np.zeros((len(lags), dim)))
    for d in range(dim):
        col = Y[:, d, :]
        out["sum"][d] = Fraction(_isum(col), den)
        out["sumsq"][d] = Fraction(_isum(col * col), den * den)
        for i, k in enumerate(lags):
            if k >= nslots:
                out["lagged"][i, d] = Fraction(0)
                continue
            out["lagged"][i, d] = Fraction(_isum(col[k:] * col[:nslots - k]), den * den)
            out["abs_lagged"][i, d] = float(np.sum(a[k:, d] * a[:nslots - k, d])) * DOWN
    return out


def check_rounding_bound(got_sum, got_sumsq, got_lagged, exact, lags, nslots, nchains, tag=""):
    """Asserts every device value within its bound of the exact one (rows beyond the trace: exactly 0) and returns the
    worst |error| / bound."""
    worst = 0.0
    n = nslots * nchains
    for d in range(len(got_sum)):
        err = abs(F(got_sum[d]) - exact["sum"][d])
        bound = 2 * gamma(n + 1) * F(exact["abs_sum"][d])
        assert err <= bound, (tag, "sum", d, float(err), float(bound))
        err = abs(F(got_sumsq[d]) - exact["sumsq"][d])
        bound = 2 * gamma(n + 2) * F(exact["abs_sumsq"][d])
        assert err <= bound, (tag, "sumsq", d, float(err), float(bound))
        for i, k in enumerate(lags):
            if k >= nslots:
                assert got_lagged[i, d] == 0.0, (tag, "lag", k, d)
                continue
            bound = 2 * gamma((nslots - k) * nchains + 2) * F(exact["abs_lagged"][i, d])
            err = abs(F(got_lagged[i, d]) - exact["lagged"][i, d])
            assert err <= bound, (tag, "lag", k, d, float(err), float(bound))
            if bound:
                worst = max(worst, float(err / bound))
    return worst
