"""The event samples and points of the device tests of SMCMC_LIKE_EVENT_TEMPLATE (tests/test_gpu_event_template*.py):
the smallest shapes at which each of the two kernels can still go wrong.

  event_template_loglike (frozen, pooled)   the fill runs twice, over [0, nsignal) and over [nsignal, nevents), in batches
                                            of four counted from the start of each pass.  (nsignal, nbackground) =
                                            (1, 1) (2, 3) (3, 2) (4, 4) (5, 1) (1, 5): the class boundary at every position of
                                            a batch of four and on a batch edge.  97 bins: the largest dynamic LDS and 291
                                            rows of the park image; 1 bin: three rows and the spare one.
  pw_event_template (SMCMC_MODE_PER_CHAIN)  22 / 64 / 65 / 86 / 97 bins: one count of owner registers each (and as many
                                            registers of the parked signal share); (1, 1) (63, 2) (64, 64) (65, 1) (2, 65)
                                            (129, 3): less than a batch of 64, exactly one, one and one, two and one, in
                                            either class.

The class counts are cut from a larger sample by event_template_ref.keep_classes; ref.truncate alone cannot choose them.
In the larger sample the background events of a mass below 300 come first (in their own order): make_sample's first
background event is the one far above xmax, and a class none of whose events survives has no finite likelihood to start
a chain from.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("smcmc_event_template_ref",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_template_ref.py"))
tref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tref)
ref, cases = tref.ref, tref.cases

NCHAINS = 130                        # the ensemble: two full wavefronts and two lanes (the park image past the first
                                     # wavefront, next to padded lanes)
ENSEMBLE_COUNTS = [(1, 1), (2, 3), (3, 2), (4, 4), (5, 1), (1, 5)]
ENSEMBLE_BINS = {"97bins": (25, 40, 97, 107), "1bin": (20, 25, 1, 110)}          # signal, background, nbins, key
PER_CHAIN_COUNTS = [(1, 1), (63, 2), (64, 64), (65, 1), (2, 65), (129, 3)]
PER_CHAIN_BINS = {"22bins": (20, 32, 22, 103), "64bins": (18, 30, 64, 104), "65bins": (25, 36, 65, 105),
                  "86bins": (30, 40, 86, 106), "97bins": (25, 40, 97, 107)}


def light_background_first(params):
    """the same sample with the background events of Mass < 300 ahead of the other background events"""
    params = np.asarray(params, dtype=np.float64)
    nev, nbins = int(params[0]), int(params[1])
    ev = params[8 + 3 * nbins:].reshape(nev, 6)
    sig, bkg = ev[ev[:, 1] <= 0], ev[ev[:, 1] > 0]
    light = bkg[:, 0] < 300.0
    return np.concatenate([params[:8 + 3 * nbins], sig.ravel(), bkg[light].ravel(), bkg[~light].ravel()])


def counted(oracle, kernel, nsignal, nbackground):
    """(nsignal, nbackground) events: of a 5-bin sample for the ensemble kernel, of a 50-bin one for the per-chain kernel"""
    base = tref.make_sample(oracle, 30, 34, 5, 102) if kernel == "ensemble" else tref.make_sample(oracle, 140, 80, 50, 111)
    return tref.keep_classes(light_background_first(base), nsignal, nbackground)


def binned(oracle, spec):
    return light_background_first(tref.make_sample(oracle, *spec))


def starts(oracle, nchains, key, params):
    """[9][nchains]: the systematic parameters uniform in (-1, 1), the two counts the sample's data total shared out and
    jittered by up to a tenth"""
    r = ref._Stream(oracle, key)
    x0 = np.array([[2.0 * r.uniform() - 1.0 for _ in range(nchains)] for _ in range(9)])
    nbins = int(params[1])
    total = float(np.sum(params[8:8 + 3 * nbins]))
    x0[0] = 0.4 * total * (1.0 + 0.1 * x0[0])
    x0[1] = 0.6 * total * (1.0 + 0.1 * x0[1])
    return x0


def forced(x0):
    """A proposal for every chain, [9][nchains]: the two extreme points of event_sample_cases (every event dropped: both
    integrals 0, NaN; every event in the first bins), a negative signal count, a negative background count, both, and
    for the other chains their start moved a little."""
    f = x0.copy()
    f[2:] += 0.01
    up, down = cases.extreme_points()
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
            self.seen[key] = self.smcmc.event_template_evaluate(self.params, point)
        return self.seen[key]


def check_forced_step(eng, x0, value, what):
    """ForceStep to forced(x0), one step: every chain's proposed likelihood is `value` at its forced point, NaN as NaN;
    returns the forced points' values"""
    f = forced(x0)
    eng.ForceStep(f)
    eng.Step(1)
    got = eng.lane("logl_proposed")
    want = np.array([value(f[:, c]) for c in range(f.shape[1])])
    for c in range(f.shape[1]):
        assert tref.same(got[c], want[c]), "%s: forced step, chain %d: %r != %r" % (what, c, got[c], want[c])
    assert np.isnan(want[0]) and np.isfinite(want[1])          # the extreme points are what they are meant to be
    return want
