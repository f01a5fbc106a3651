"""SMCMC_LIKE_EVENT_SHAPE on the device, every branch of the two kernels, on the samples of tests/event_shape_cases.py
(which says what each shape is for).  Every likelihood the device reports is smcmc.event_shape_evaluate -- the host
definition, which tests/test_event_shape_cpu.py pins to the restatement bit for bit and
tests/test_event_shape_truth_cpu.py to the definition in high precision -- at the point it reports, bit for bit and NaN
as NaN.  Beside the chains' own steps every engine takes one forced step to the two extreme points (every event dropped:
both integrals 0 and the likelihood NaN, on host and device alike; every event in the first bins), to a negative signal
count, a negative background count and both.  Every sample has an event of each class with a separation exactly on
each cut, and -- from eleven events per class on -- masses on every branch of the shape's rule."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_event_shape_cases", os.path.join(HERE, "event_shape_cases.py"))
scases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(scases)
sref, ref = scases.sref, scases.ref

pytestmark = pytest.mark.gpu
SEED = 20260131
NCHAINS = scases.NCHAINS
DIM = 31


def test_the_maximum_is_the_librarys(gpu):
    assert scases.MAX_BINS == gpu._capi.EVENT_SHAPE_MAX_BINS >= 50


def _ensemble(gpu, oracle, params, mode, what):
    host = scases.Host(gpu, params)
    eng = gpu.Engine(DIM, nchains=NCHAINS, likelihood=gpu.LIKE_EVENT_SHAPE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_FROZEN if mode == "frozen" else gpu.MODE_POOLED)
    eng.KeepProposed()
    x0 = scases.starts(oracle, NCHAINS, 77, params)
    assert eng.Start(x0), what
    logl = eng.lane("logl")
    for c in range(NCHAINS):
        assert logl[c] == host(x0[:, c]), "%s: start, chain %d" % (what, c)
    scases.check_forced_step(eng, x0, host, what, params)
    if mode == "frozen":
        eng.Step(16)
    else:
        eng.sync()
        eng.Step(15)
        eng.sync()
    x, xp = eng.GetAccepted(), eng.GetProposed()
    logl, loglp = eng.lane("logl"), eng.lane("logl_proposed")
    for c in range(NCHAINS):
        assert logl[c] == host(x[:, c]), "%s: accepted, chain %d" % (what, c)
        assert sref.same(loglp[c], host(xp[:, c])), "%s: proposed, chain %d" % (what, c)
    assert int(eng.lane("naccept").sum()) > 0 and not np.array_equal(x, x0)
    hist, l2 = eng.EventShapeHistograms(x[:, 2])
    assert l2 == logl[2] and hist.shape == (4, int(params[1]))
    eng.close()


@pytest.mark.parametrize("mode", ["frozen", "pooled"])
@pytest.mark.parametrize("name", list(scases.ENSEMBLE_BINS))
def test_ensemble_kernel_bin_counts(gpu, oracle, name, mode):
    """the maximum with the moment fold (pooled) and without (frozen): the largest dynamic LDS beside either static LDS"""
    params = scases.with_separations_on_the_cuts(scases.binned(oracle, scases.ENSEMBLE_BINS[name]))
    _ensemble(gpu, oracle, params, mode, name)


@pytest.mark.parametrize("counts", scases.ENSEMBLE_COUNTS, ids=lambda c: "%dsig_%dbkg" % c)
def test_ensemble_kernel_class_boundary(gpu, oracle, counts):
    params = scases.counted(oracle, "ensemble", *counts)
    _ensemble(gpu, oracle, params, "frozen", "%d + %d events" % counts)


def _per_chain(gpu, oracle, params, what):
    host = scases.Host(gpu, params)
    nchains, nsteps = 5, 16
    eng = gpu.Engine(DIM, nchains=nchains, likelihood=gpu.LIKE_EVENT_SHAPE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_PER_CHAIN)
    assert eng.get_param("PERCHAIN_WAVE") == 1.0
    x0 = scases.starts(oracle, nchains, 78, params)
    assert eng.Start(x0), what
    start_logl = eng.lane("logl")
    for c in range(nchains):
        assert start_logl[c] == host(x0[:, c]), "%s: start, chain %d" % (what, c)
    hist, l0 = eng.EventShapeHistograms(x0[:, 0])
    assert l0 == start_logl[0] and hist.shape == (4, int(params[1]))
    eng.snapshot()
    scases.check_forced_step(eng, x0, host, what, params)
    eng.rollback()
    moved = 0
    for c in range(3):
        rec = eng.StepRecorded(nsteps, chain=c)
        for s in range(nsteps):
            assert sref.same(rec["logl_proposed"][s], host(rec["proposed"][s])), "%s: proposed, chain %d step %d" % (what, c, s)
            assert rec["logl"][s] == host(rec["accepted"][s]), "%s: accepted, chain %d step %d" % (what, c, s)
        moved += int(rec["last_accept"].sum())
        eng.rollback()
    assert moved > 0
    eng.close()


@pytest.mark.parametrize("name", list(scases.PER_CHAIN_BINS))
def test_per_chain_wave_kernel_bin_counts(gpu, oracle, name):
    params = scases.with_separations_on_the_cuts(scases.binned(oracle, scases.PER_CHAIN_BINS[name]))
    _per_chain(gpu, oracle, params, name)


@pytest.mark.parametrize("counts", scases.PER_CHAIN_COUNTS, ids=lambda c: "%dsig_%dbkg" % c)
def test_per_chain_wave_kernel_class_boundary(gpu, oracle, counts):
    params = scases.counted(oracle, "per_chain", *counts)
    _per_chain(gpu, oracle, params, "%d + %d events" % counts)
