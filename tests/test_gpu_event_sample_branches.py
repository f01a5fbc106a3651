"""SMCMC_LIKE_EVENT_SAMPLE on the device, every branch of the two kernels: the samples of tests/event_sample_cases.py,
whose host values tests/test_event_sample_truth_cpu.py pins to the definition in high precision.  Every likelihood the
device reports is smcmc.event_sample_evaluate -- the host definition -- at the point it reports, bit for bit, and
EventSampleHistograms gives that evaluation's bins.

  pw_event_sample (SMCMC_MODE_PER_CHAIN)   `switch (nown)`: 22 bins case 2, 64 bins case 3 at its upper edge, 65 bins
                                           case 4, 86 and 97 bins the default; 97 bins is also where the ordered bin sum
                                           reads furthest past `rows`; 1, 37, 63 events: less than one batch of 64; 65,
                                           129: batches plus one; 1 025 chains: the paired form of the kernel
  event_sample_loglike (frozen, pooled)    97 bins: the largest dynamic LDS; 1 bin: three rows and the spare row, where
                                           a batch of four holds every shape of equal indices; 1, 2, 3 events: no full
                                           batch; 5: one and one
  both                                     MassScale = 80: every event dropped, every bin clamped;  MassScale = -80:
                                           every event in the first bin of its histogram"""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("smcmc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref, cases = _load("event_sample_ref"), _load("event_sample_cases")

pytestmark = pytest.mark.gpu
SEED = 20260131
NCHAINS = 130                                        # the ensemble: two full wavefronts and two lanes


class Host:
    """the host definition of one sample, remembered by point"""
    def __init__(self, smcmc, params):
        self.smcmc, self.params, self.seen = smcmc, params, {}

    def __call__(self, point):
        key = np.asarray(point, dtype=np.float64).tobytes()
        if key not in self.seen:
            self.seen[key] = self.smcmc.event_sample_evaluate(self.params, point)
        return self.seen[key]


def _starts(oracle, nchains, key):
    """uniform in (-1, 1), the first two chains at the two extreme points"""
    r = ref._Stream(oracle, key)
    x0 = np.array([[2.0 * r.uniform() - 1.0 for _ in range(nchains)] for _ in range(9)])
    x0[:, 0], x0[:, 1] = cases.extreme_points()
    return x0


def _check_extreme_points(gpu, eng, params, start_logl):
    """chains 0 and 1 started at them"""
    nbins = int(params[1])
    up, down = cases.extreme_points()
    hist, logl = eng.EventSampleHistograms(up)
    assert not hist.any() and logl == start_logl[0]                      # all dropped: every bin clamped to 0.001
    hist, logl = eng.EventSampleHistograms(down)
    assert hist.shape == (3, nbins) and logl == start_logl[1]
    where = set(cases.host_where(gpu, params, down))
    assert where <= {0, nbins, 2 * nbins} and set(np.flatnonzero(hist.ravel())) == where


@pytest.mark.parametrize("name", cases.PER_CHAIN)
def test_per_chain_wave_kernel_is_the_host_definition(gpu, oracle, name):
    params = cases.sample(ref, oracle, name)
    host = Host(gpu, params)
    nchains, nsteps = 3, 32
    eng = gpu.Engine(9, nchains=nchains, likelihood=gpu.LIKE_EVENT_SAMPLE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_PER_CHAIN)
    assert eng.get_param("PERCHAIN_WAVE") == 1.0
    r = ref._Stream(oracle, 78)
    x0 = np.array([[2.0 * r.uniform() - 1.0 for _ in range(nchains)] for _ in range(9)])
    assert eng.Start(x0)
    start_logl = eng.lane("logl")
    for c in range(nchains):
        assert start_logl[c] == host(x0[:, c]), "start, chain %d" % c
    hist, l0 = eng.EventSampleHistograms(x0[:, 0])
    assert l0 == start_logl[0] and hist.shape == (3, int(params[1]))
    eng.snapshot()
    moved = 0
    for c in range(nchains):
        rec = eng.StepRecorded(nsteps, chain=c)
        for s in range(nsteps):
            assert rec["logl_proposed"][s] == host(rec["proposed"][s]), "proposed, chain %d step %d" % (c, s)
            assert rec["logl"][s] == host(rec["accepted"][s]), "accepted, chain %d step %d" % (c, s)
        moved += int(rec["last_accept"].sum())
        eng.rollback()
    assert moved > 0
    eng.close()


@pytest.mark.parametrize("name", ["65ev_97bins", "129ev_50bins", "1ev_50bins"])
def test_per_chain_wave_kernel_at_the_extreme_points(gpu, oracle, name):
    params = cases.sample(ref, oracle, name)
    eng = gpu.Engine(9, nchains=3, likelihood=gpu.LIKE_EVENT_SAMPLE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_PER_CHAIN)
    assert eng.Start(_starts(oracle, 3, 79))
    _check_extreme_points(gpu, eng, params, eng.lane("logl"))
    eng.close()


def test_per_chain_wave_kernel_paired_form_above_1024_chains(gpu, oracle):
    """1 025 chains: the first count at which the per-chain wave kernel is launched in its paired form
    (perchain_wave_kernel<EVENT_SAMPLE, 4, PAIRED = true>), which no other event test reaches.  65 signal and 2
    background events: a second batch of 64 that holds one event; 22 bins: 66 rows, two owner registers.  Start, then two
    steps: every chain's start and accepted likelihood is the host definition at its point, bit for bit and NaN as NaN,
    and for chains 0, 1 and 1 024 the Python restatement's too."""
    tref = _load("event_template_ref")                   # (keep_classes: ref.truncate cannot choose the class counts)
    params = tref.keep_classes(ref.make_sample(oracle, 70, 8, 22, 112), 65, 2)
    assert tref.class_counts(params) == (65, 2)
    host, be = Host(gpu, params), ref.deterministic(oracle, gpu)
    nchains = 1025
    eng = gpu.Engine(9, nchains=nchains, likelihood=gpu.LIKE_EVENT_SAMPLE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_PER_CHAIN)
    assert eng.get_param("PERCHAIN_WAVE") == 1.0
    x0 = np.random.default_rng(80).uniform(-1.0, 1.0, (9, nchains))
    assert eng.Start(x0)
    for when, steps in (("start", 0), ("accepted", 2)):
        if steps:
            eng.Step(steps)
        x, logl = eng.GetAccepted(), eng.lane("logl")
        assert logl.shape == (nchains,)
        for c in range(nchains):
            assert tref.same(logl[c], host(x[:, c])), "%s, chain %d" % (when, c)
        for c in (0, 1, 1024):
            assert tref.same(logl[c], ref.evaluate(params, x[:, c], be)[0]), "%s, chain %d: the restatement" % (when, c)
    assert not np.array_equal(x, x0)
    eng.close()


@pytest.mark.parametrize("mode", ["frozen", "pooled"])
@pytest.mark.parametrize("name", cases.ENSEMBLE)
def test_ensemble_kernel_is_the_host_definition(gpu, oracle, name, mode):
    params = cases.sample(ref, oracle, name)
    host = Host(gpu, params)
    eng = gpu.Engine(9, nchains=NCHAINS, likelihood=gpu.LIKE_EVENT_SAMPLE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_FROZEN if mode == "frozen" else gpu.MODE_POOLED)
    eng.KeepProposed()
    x0 = _starts(oracle, NCHAINS, 77)
    assert eng.Start(x0)
    logl = eng.lane("logl")
    assert np.array_equal(eng.GetAccepted(), x0)
    for c in range(NCHAINS):
        assert logl[c] == host(x0[:, c]), "start, chain %d" % c
    _check_extreme_points(gpu, eng, params, logl)
    if mode == "frozen":
        eng.Step(32)
    else:
        for _ in range(2):                           # 32 steps, a sync every 16
            eng.Step(16)
            eng.sync()
    x, xp = eng.GetAccepted(), eng.GetProposed()
    logl, loglp = eng.lane("logl"), eng.lane("logl_proposed")
    for c in range(NCHAINS):
        assert logl[c] == host(x[:, c]), "accepted, chain %d" % c
        assert loglp[c] == host(xp[:, c]), "proposed, chain %d" % c
    assert int(eng.lane("naccept").sum()) > 0 and not np.array_equal(x, x0)
    hist, l2 = eng.EventSampleHistograms(x[:, 2])
    assert l2 == logl[2] and hist.shape == (3, int(params[1]))
    eng.close()


def _shape(idx):
    """a batch's rows up to renaming: (7, 7, 2, 7) is aaba"""
    names = {}
    return "".join(names.setdefault(i, "abcd"[len(names)]) for i in idx)


def test_the_ensemble_batches_hold_every_shape_of_equal_rows(gpu, oracle):
    """event_sample_loglike forwards a bin's running sum inside a batch of four when two of its events hit the same row.
    The start points of test_ensemble_kernel_is_the_host_definition (each evaluated by Start and compared above) hold
    batches of four with all four rows equal, two pairs in each of the three arrangements, and a repeat across two
    others.  From the host's `where`; a dropped event goes to the spare row behind the last bin."""
    seen = set()
    x0 = _starts(oracle, NCHAINS, 77)
    for name in ("45ev_1bin", "5ev_5bins"):
        params = cases.sample(ref, oracle, name)
        rows, nev = 3 * int(params[1]), int(params[0])
        for c in range(8):
            where = [k if k >= 0 else rows for k in cases.host_where(gpu, params, x0[:, c])]
            seen |= {_shape(where[e:e + 4]) for e in range(0, nev - 3, 4)}
    print("shapes of the full batches:", " ".join(sorted(seen)))
    assert {"aaaa", "aabb", "abab", "abba", "abca"} <= seen
