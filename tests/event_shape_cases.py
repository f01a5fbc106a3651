"""The event samples and points of the device tests of SMCMC_LIKE_EVENT_SHAPE (tests/test_gpu_event_shape*.py): the
smallest shapes at which each of the two kernels can still go wrong.

  event_shape_loglike (frozen, pooled)   the fill runs twice, over [0, nsignal) and over [nsignal, nevents), in batches of
                                         four counted from the start of each pass.  (nsignal, nbackground) = (1, 1) (2, 3)
                                         (3, 2) (4, 4) (5, 1) (1, 5): the class boundary at every position of a batch of
                                         four and on a batch edge.  SMCMC_EVENT_SHAPE_MAX_BINS: the largest dynamic LDS
                                         (histograms, spare row, tables) and the most rows of the park image; 1 bin: four
                                         rows and the spare one.
  pw_event_shape (SMCMC_MODE_PER_CHAIN)  16 / 17 / 32 / 33 / 48 / 49 / 50 / the maximum: 4 nbins on both sides of every
                                         multiple of 64, so every count of owner registers and both sides of each; (1, 1)
                                         (63, 2) (64, 64) (65, 1) (2, 65) (129, 3): less than a batch of 64, exactly one,
                                         one and one, two and one, in either class.

Every sample of event_shape_ref.make_sample with at least 11 events per class carries the masses of
event_shape_ref.shape_masses(): each branch of the shape's rule in both classes.  The class counts are cut from a larger
sample by keep_classes; in it the background events of a mass below 300 come first, so that no start point is left
without a surviving event in a class.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("smcmc_event_shape_ref",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_shape_ref.py"))
sref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sref)
ref = sref.ref

MAX_BINS = 59                        # SMCMC_EVENT_SHAPE_MAX_BINS (the tests assert it against the package's)
NCHAINS = 130                        # the ensemble: two full wavefronts and two lanes (the park image past the first
                                     # wavefront, next to padded lanes)
ENSEMBLE_COUNTS = [(1, 1), (2, 3), (3, 2), (4, 4), (5, 1), (1, 5)]
ENSEMBLE_BINS = {"maxbins": (25, 40, MAX_BINS, 207), "1bin": (20, 25, 1, 210)}          # signal, background, nbins, key
PER_CHAIN_COUNTS = [(1, 1), (63, 2), (64, 64), (65, 1), (2, 65), (129, 3)]
PER_CHAIN_BINS = {"%dbins" % n: (20 + n % 7, 30 + n % 5, n, 220 + n) for n in (16, 17, 32, 33, 48, 49, 50, MAX_BINS)}


def counted(oracle, kernel, nsignal, nbackground):
    """(nsignal, nbackground) events: of a 5-bin sample for the ensemble kernel, of a 50-bin one for the per-chain kernel"""
    base = sref.make_sample(oracle, 30, 34, 5, 202) if kernel == "ensemble" else sref.make_sample(oracle, 140, 80, 50, 211)
    return sref.keep_classes(sref.light_background_first(base), nsignal, nbackground)


def binned(oracle, spec):
    return sref.light_background_first(sref.make_sample(oracle, *spec))


def with_separations_on_the_cuts(params):
    """the same sample with an untagged event of each class exactly on each cut: 50 (Close, not VeryClose) and 100
    (Separated, not Close)"""
    params = np.array(params, dtype=np.float64)
    at = sref.events_offset(params)
    ev = params[at:].reshape(-1, 6)
    sig, bkg = np.flatnonzero(ev[:, 1] <= 0), np.flatnonzero(ev[:, 1] > 0)
    for rows in (sig, bkg):
        assert len(rows) >= 2
        ev[rows[0], 2], ev[rows[0], 3] = 50.0, 0
        ev[rows[1], 2], ev[rows[1], 3] = 100.0, 0
    return params


def starts(oracle, nchains, key, params):
    """[31][nchains]: the systematic and the shape parameters uniform in (-1, 1), the two counts the sample's data total
    shared out and jittered by up to a tenth"""
    r = ref._Stream(oracle, key)
    x0 = np.array([[2.0 * r.uniform() - 1.0 for _ in range(nchains)] for _ in range(31)])
    total = sref.data_total(params)
    x0[0] = 0.4 * total * (1.0 + 0.1 * x0[0])
    x0[1] = 0.6 * total * (1.0 + 0.1 * x0[1])
    return x0


def forced(x0, params):
    """A proposal for every chain, [31][nchains]: the two extreme points (every event dropped: both integrals 0, NaN; every
    event in the first bins), a negative signal count, a negative background count, both, and for the other chains their
    start moved a little.  With separation scales of zero (chains 0 and 1) a separation on a cut stays on it."""
    f = x0.copy()
    f[2:] += 0.01
    up, down = sref.extreme_points(params)
    for k, p in enumerate((up, down)):
        f[:, k] = p
        f[0, k], f[1, k] = x0[0, k], x0[1, k]
    if f.shape[1] > 2:
        f[0, 2] = -f[0, 2]
    if f.shape[1] > 3:
        f[1, 3] = -f[1, 3]
    if f.shape[1] > 4:
        f[0, 4], f[1, 4] = -f[0, 4], -f[1, 4]
    return f


class Host:
    """the host definition of one sample, remembered by point"""
    def __init__(self, smcmc, params):
        self.smcmc, self.params, self.seen = smcmc, params, {}

    def __call__(self, point):
        key = np.asarray(point, dtype=np.float64).tobytes()
        if key not in self.seen:
            self.seen[key] = self.smcmc.event_shape_evaluate(self.params, point)
        return self.seen[key]


def check_forced_step(eng, x0, value, what, params):
    """ForceStep to forced(x0), one step: every chain's proposed likelihood is `value` at its forced point, NaN as NaN;
    returns the forced points' values"""
    f = forced(x0, params)
    eng.ForceStep(f)
    eng.Step(1)
    got = eng.lane("logl_proposed")
    want = np.array([value(f[:, c]) for c in range(f.shape[1])])
    for c in range(f.shape[1]):
        assert sref.same(got[c], want[c]), "%s: forced step, chain %d: %r != %r" % (what, c, got[c], want[c])
    assert np.isnan(want[0]) and np.isfinite(want[1])          # the extreme points are what they are meant to be
    return want
