"""The event samples shared by tests/test_event_sample_truth_cpu.py (host definition against the high-precision truth)
and tests/test_gpu_event_sample_branches.py (device against the host definition): one sample per branch of the two
device kernels, so that every configuration the device is asked for is one whose host value the truth has pinned.

  nbins   rows = 3 nbins   registers of a bin owner in pw_event_sample (ceil(rows / 64))
  1       3                1      (and in event_sample_loglike: three rows and the spare one)
  5       15               1
  22      66               2      the smallest count that needs two
  50      150              3
  64      192              3      the largest count that needs three
  65      195              4      the smallest that needs four
  86      258              5      the smallest that needs five
  97      291              5      SMCMC_EVENT_SAMPLE_MAX_BINS: the largest dynamic LDS of event_sample_loglike, and the
                                  bin sum of pw_event_sample reading furthest past `rows`

The event counts: below one batch of the per-chain kernel (1, 37, 63 of 64), one batch plus one (65), two plus one (129);
below one batch of the ensemble kernel (1, 2, 3 of 4) and one plus one (5).  make_sample needs two signal and three
background events, so these are the first events of a larger sample (ref.truncate)."""
import numpy as np

# name: (nsignal, nbackground, nbins, key, nevents kept or None for all, exposure ratio)
CASES = {
    "197ev_50bins": (60, 137, 50, 101, None, 1.0),          # the two of tests/test_event_sample_cpu.py
    "64ev_5bins": (30, 34, 5, 102, None, 1.0),
    "52ev_22bins": (20, 32, 22, 103, None, 0.731),
    "48ev_64bins": (18, 30, 64, 104, None, 1.0),
    "61ev_65bins": (25, 36, 65, 105, None, 1.37),
    "70ev_86bins": (30, 40, 86, 106, None, 1.0),
    "65ev_97bins": (25, 40, 97, 107, None, 0.9),
    "45ev_1bin": (20, 25, 1, 110, None, 2.3),    # (a key whose batches of four hold every shape of equal rows)
    "1ev_50bins": (60, 137, 50, 101, 1, 1.0),
    "37ev_50bins": (60, 137, 50, 101, 37, 1.0),
    "63ev_50bins": (60, 137, 50, 101, 63, 1.0),
    "65ev_50bins": (60, 137, 50, 101, 65, 1.0),
    "129ev_50bins": (60, 137, 50, 101, 129, 1.0),
    "1ev_5bins": (30, 34, 5, 102, 1, 1.0),
    "2ev_5bins": (30, 34, 5, 102, 2, 1.0),
    "3ev_5bins": (30, 34, 5, 102, 3, 1.0),
    "5ev_5bins": (30, 34, 5, 102, 5, 1.0),
}
NPOINTS = 12

# the per-chain wave kernel: every count of owner registers, and the event counts around its batch of 64
PER_CHAIN = ["52ev_22bins", "48ev_64bins", "61ev_65bins", "70ev_86bins", "65ev_97bins",
             "1ev_50bins", "37ev_50bins", "63ev_50bins", "65ev_50bins", "129ev_50bins"]
# the ensemble kernel: the largest and the smallest histogram, and the event counts around its batch of four
ENSEMBLE = ["65ev_97bins", "45ev_1bin", "1ev_5bins", "2ev_5bins", "3ev_5bins", "5ev_5bins"]


def sample(ref, oracle, name):
    nsig, nbkg, nbins, key, keep, exposure = CASES[name]
    params = ref.make_sample(oracle, nsig, nbkg, nbins, key)
    params[4] = exposure
    return params if keep is None else ref.truncate(params, keep)


def points(ref, oracle, name):
    return ref.points(oracle, NPOINTS, CASES[name][3] + 1000)


def extreme_points():
    """MassScale = +-80: every mass times e^8, so every event is above 500, dropped, and every bin is clamped; every mass
    times e^-8, so every event is in the first bin of its histogram"""
    up, down = np.zeros(9), np.zeros(9)
    up[2], down[2] = 80.0, -80.0
    return up, down


def one_event(params, i):
    """the sample that holds event i alone"""
    params = np.asarray(params, dtype=np.float64)
    ev0 = 8 + 3 * int(params[1])
    out = np.concatenate([params[:ev0], params[ev0 + 6 * i:ev0 + 6 * i + 6]])
    out[0] = 1.0
    return out


def host_where(smcmc, params, point):
    """Where the host definition puts each event: an event's bin and weight do not depend on the other events, so the
    one bin that is not zero when the event is evaluated alone is its bin, and none means a cut or the axis dropped it
    (-1).  A weight is never zero: it is a product of exponentials, of a probability inside (0, 1) and of the exposure."""
    where = []
    for i in range(int(params[0])):
        _, hist = smcmc.event_sample_evaluate(one_event(params, i), point, histograms=True)
        hit = np.flatnonzero(hist.ravel())
        assert hit.size <= 1
        where.append(int(hit[0]) if hit.size else -1)
    return where
