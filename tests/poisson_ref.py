"""The Poisson variate of include/smcmc_poisson.h restated in Python floats from the header's comment, line by line.

IEEE binary64, un-fused, is what Python's float arithmetic is; math.sqrt is the correctly rounded root.  The two things
the header takes from elsewhere are taken from their own checked sources: the Philox block from the CPU oracle's
draw_block, exp from the library's host smcmc_exp (smcmc_selftest_detmath on device -1, kind 1).
"""
import math

import numpy as np

MAX_MEAN = 1048576.0
MIN_MEAN, SPLIT = 0.001, 16.0
SMALL_STEPS, BD0_TERMS, TAIL_STEPS = 1024, 16, 2048
STREAM_REPLICA = 5


def valid(expectation):
    return not math.isnan(expectation) and not math.isinf(expectation) and expectation <= MAX_MEAN


def mean_of(expectation):
    return MIN_MEAN if expectation < MIN_MEAN else expectation


def step_of(slot, row, replica):
    return slot | (row << 28) | (replica << 44)


def uniform_of(w0, w1):
    n = (w0 << 20) | (w1 >> 12)
    return (float(n) + 0.5) * 2.0 ** -52


def stirlerr(m):
    m2 = m * m
    return (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) / m2) / m2) / m2) / m2) / m


def bd0(m, mu):
    d = m - mu
    v = d / (m + mu)
    s = d * v
    e = (2.0 * m) * v
    v = v * v
    for j in range(1, BD0_TERMS + 1):
        e = e * v
        s1 = s + e / float(2 * j + 1)
        if s1 == s:
            return s1
        s = s1
    return s


class Restatement:
    """oracle: the CPU oracle module (draw_block); smcmc: the package (the host exp)"""

    def __init__(self, oracle, smcmc):
        self._block = oracle.draw_block
        self._exp = lambda x: float(smcmc.selftest_detmath(1, np.array([x]), device=-1)[0])
        self._start = {}

    def uniform_at(self, seed, chain, slot, row, replica):
        w = self._block(seed, chain, step_of(slot, row, replica), 0, STREAM_REPLICA)
        return uniform_of(w[0], w[1])

    def _first_term(self, mu):
        """the term the inversion starts from: a function of the mean alone, so taken once per mean"""
        if mu not in self._start:
            if mu < SPLIT:
                self._start[mu] = self._exp(-mu)
            else:
                m = float(int(mu))
                self._start[mu] = self._exp(-stirlerr(m) - bd0(m, mu)) / math.sqrt(6.283185307179586 * m)
        return self._start[mu]

    def from_uniform(self, expectation, u):
        mu = mean_of(expectation)
        p = self._first_term(mu)
        if mu < SPLIT:
            k = 0
            while k < SMALL_STEPS:
                u -= p
                if u <= 0.0:
                    return float(k)
                k += 1
                p = (p * mu) / float(k)
                if p == 0.0 and float(k) > mu:
                    return float(k)
            return float(SMALL_STEPS)
        mi = int(mu)
        u -= p
        if u <= 0.0:
            return float(mi)
        pu = pd = p
        last = mi + TAIL_STEPS
        for t in range(1, last + 1):
            pu = (pu * mu) / float(mi + t)
            u -= pu
            if u <= 0.0:
                return float(mi + t)
            if t <= mi:
                pd = (pd * float(mi - t + 1)) / mu
                u -= pd
                if u <= 0.0:
                    return float(mi - t)
            elif pu < 1e-300:
                return float(mi + t)
        return float(mi + last)

    def draw(self, seed, chain, slot, row, replica, expectation):
        """(y, valid)"""
        if not valid(expectation):
            return float("nan"), 0
        return self.from_uniform(expectation, self.uniform_at(seed, chain, slot, row, replica)), 1
