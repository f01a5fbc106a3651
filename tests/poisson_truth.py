"""Independent truth for the Poisson variate of include/smcmc_poisson.h: the thresholds of the cumulative distribution.

The variate is inversion: with the indices taken in the definition's order (0, 1, 2, ... below a mean of 16; m, m + 1,
m - 1, m + 2, m - 2, ... from the mode m = floor(mu) from 16 up) and c_i the sum of the first i + 1 probabilities, the
uniform u gives the first index whose c_i >= u.  Here every probability is the exact mass function
    exp(-mu + k ln mu - lgamma(k + 1))
in mpmath at 256 bits, term by term, and the c_i are their running sum: no recurrence, no Stirling series, no code of the
header or of tests/poisson_ref.py.  A threshold rounded to binary64 is within 1.2e-16 of the exact one, far inside the
1e-10 band the comparison leaves out, so the search runs on doubles.
"""
import mpmath as mp
import numpy as np

PREC = 256
BAND = 1e-10
MIN_MEAN, SPLIT = 0.001, 16.0


def mean_of(expectation):
    """the mean the variate is drawn at: the clamp of the likelihood's bin term"""
    return MIN_MEAN if expectation < MIN_MEAN else float(expectation)


def order(mu, count):
    """the first `count` indices in the definition's order"""
    if mu < SPLIT:
        return list(range(count))
    m = int(mp.floor(mp.mpf(mu)))
    out, t = [m], 1
    while len(out) < count:
        out.append(m + t)
        if m - t >= 0 and len(out) < count:
            out.append(m - t)
        t += 1
    return out


def thresholds(mu):
    """(indices, c): the indices in the definition's order and the cumulative sums of the exact mass function over them,
    as doubles, up to the first sum within 2^-60 of one (the largest uniform is 1 - 2^-53)"""
    with mp.workprec(PREC):
        mu = mp.mpf(mu)
        lnmu = mp.log(mu)
        sd = float(mp.sqrt(mu))
        count = int(float(mu) + 64) if mu < SPLIT else int(2 * 9.5 * sd + 64)
        eps = mp.mpf(2) ** -60
        while True:
            idx = order(float(mu), count)
            c, total = [], mp.mpf(0)
            for k in idx:
                total += mp.exp(-mu + k * lnmu - mp.loggamma(k + 1))
                c.append(float(total))
                if 1 - total < eps:
                    break
            if 1 - total < eps:
                return np.array(idx[:len(c)], dtype=np.int64), np.array(c)
            count *= 2


def check(u, drawn, mu):
    """The draws `drawn` of the uniforms `u` against the truth at mean `mu`: (mismatches, excluded, thresholds): the number
    of draws outside the band that are not the truth's index, the number left out because u is within BAND of a
    neighbouring threshold, and the number of thresholds."""
    idx, c = thresholds(mu)
    u, drawn = np.asarray(u, dtype=np.float64), np.asarray(drawn, dtype=np.float64)
    at = np.searchsorted(c, u, side="left")                      # the first c_i >= u
    assert at.max() < len(c), "a uniform beyond the last threshold"
    upper = c[at]
    lower = np.where(at > 0, c[np.maximum(at - 1, 0)], -1.0)
    near = (np.abs(u - upper) <= BAND) | (np.abs(u - lower) <= BAND)
    wrong = (~near) & (drawn != idx[at].astype(np.float64))
    return int(wrong.sum()), int(near.sum()), len(c)
