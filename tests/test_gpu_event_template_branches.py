"""SMCMC_LIKE_EVENT_TEMPLATE on the device, every branch of the two kernels, on the samples of
tests/event_template_cases.py (which says what each shape is for).  Every likelihood the device reports is
smcmc.event_template_evaluate -- the host definition, which tests/test_event_template_truth_cpu.py pins to the definition
in high precision -- at the point it reports, bit for bit and NaN as NaN.  Beside the chains' own steps every engine
takes one forced step to the two extreme points (every event dropped: both integrals 0 and the likelihood NaN, on host
and device alike; every event in the first bins), to a negative signal count, a negative background count and both."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_event_template_cases", os.path.join(HERE, "event_template_cases.py"))
tcases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tcases)
tref, ref = tcases.tref, tcases.ref

pytestmark = pytest.mark.gpu
SEED = 20260131
NCHAINS = tcases.NCHAINS


def _ensemble(gpu, oracle, params, mode, what):
    host = tcases.Host(gpu, params)
    eng = gpu.Engine(9, nchains=NCHAINS, likelihood=gpu.LIKE_EVENT_TEMPLATE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_FROZEN if mode == "frozen" else gpu.MODE_POOLED)
    eng.KeepProposed()
    x0 = tcases.starts(oracle, NCHAINS, 77, params)
    assert eng.Start(x0), what
    logl = eng.lane("logl")
    for c in range(NCHAINS):
        assert logl[c] == host(x0[:, c]), "%s: start, chain %d" % (what, c)
    tcases.check_forced_step(eng, x0, host, what)
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
        assert tref.same(loglp[c], host(xp[:, c])), "%s: proposed, chain %d" % (what, c)
    assert int(eng.lane("naccept").sum()) > 0 and not np.array_equal(x, x0)
    hist, l2 = eng.EventTemplateHistograms(x[:, 2])
    assert l2 == logl[2] and hist.shape == (3, int(params[1]))
    eng.close()


@pytest.mark.parametrize("mode", ["frozen", "pooled"])
@pytest.mark.parametrize("name", list(tcases.ENSEMBLE_BINS))
def test_ensemble_kernel_bin_counts(gpu, oracle, name, mode):
    """97 bins with the moment fold (pooled) and without (frozen): the largest dynamic LDS beside either static LDS"""
    _ensemble(gpu, oracle, tcases.binned(oracle, tcases.ENSEMBLE_BINS[name]), mode, name)


@pytest.mark.parametrize("counts", tcases.ENSEMBLE_COUNTS, ids=lambda c: "%dsig_%dbkg" % c)
def test_ensemble_kernel_class_boundary(gpu, oracle, counts):
    params = tcases.counted(oracle, "ensemble", *counts)
    assert tref.class_counts(params) == counts
    _ensemble(gpu, oracle, params, "frozen", "%d + %d events" % counts)


def _per_chain(gpu, oracle, params, what):
    host = tcases.Host(gpu, params)
    nchains, nsteps = 5, 16
    eng = gpu.Engine(9, nchains=nchains, likelihood=gpu.LIKE_EVENT_TEMPLATE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_PER_CHAIN)
    assert eng.get_param("PERCHAIN_WAVE") == 1.0
    x0 = tcases.starts(oracle, nchains, 78, params)
    assert eng.Start(x0), what
    start_logl = eng.lane("logl")
    for c in range(nchains):
        assert start_logl[c] == host(x0[:, c]), "%s: start, chain %d" % (what, c)
    hist, l0 = eng.EventTemplateHistograms(x0[:, 0])
    assert l0 == start_logl[0] and hist.shape == (3, int(params[1]))
    eng.snapshot()
    tcases.check_forced_step(eng, x0, host, what)
    eng.rollback()
    moved = 0
    for c in range(3):
        rec = eng.StepRecorded(nsteps, chain=c)
        for s in range(nsteps):
            assert tref.same(rec["logl_proposed"][s], host(rec["proposed"][s])), "%s: proposed, chain %d step %d" % (what, c, s)
            assert rec["logl"][s] == host(rec["accepted"][s]), "%s: accepted, chain %d step %d" % (what, c, s)
        moved += int(rec["last_accept"].sum())
        eng.rollback()
    assert moved > 0
    eng.close()


@pytest.mark.parametrize("name", list(tcases.PER_CHAIN_BINS))
def test_per_chain_wave_kernel_bin_counts(gpu, oracle, name):
    _per_chain(gpu, oracle, tcases.binned(oracle, tcases.PER_CHAIN_BINS[name]), name)


@pytest.mark.parametrize("counts", tcases.PER_CHAIN_COUNTS, ids=lambda c: "%dsig_%dbkg" % c)
def test_per_chain_wave_kernel_class_boundary(gpu, oracle, counts):
    params = tcases.counted(oracle, "per_chain", *counts)
    assert tref.class_counts(params) == counts
    _per_chain(gpu, oracle, params, "%d + %d events" % counts)


def test_per_chain_wave_kernel_paired_form_above_1024_chains(gpu, oracle):
    """1 025 chains: the first count at which the per-chain wave kernel is launched in its paired form
    (perchain_wave_kernel<EVENT_TEMPLATE, 4, PAIRED = true>), which no other event test reaches.  65 signal and 2
    background events: a second batch of 64 of the signal's scan that holds one event; 22 bins: 66 rows, two owner
    registers.  Start, then two steps: every chain's start and accepted likelihood is the host definition at its point,
    bit for bit and NaN as NaN, and for chains 0, 1 and 1 024 the Python restatement's too."""
    params = tref.keep_classes(tcases.light_background_first(tref.make_sample(oracle, 70, 8, 22, 112)), 65, 2)
    assert tref.class_counts(params) == (65, 2)
    host, be = tcases.Host(gpu, params), ref.deterministic(oracle, gpu)
    nchains = 1025
    eng = gpu.Engine(9, nchains=nchains, likelihood=gpu.LIKE_EVENT_TEMPLATE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_PER_CHAIN)
    assert eng.get_param("PERCHAIN_WAVE") == 1.0
    x0 = np.random.default_rng(81).uniform(-1.0, 1.0, (9, nchains))
    total = float(np.sum(params[8:8 + 3 * 22]))             # the two counts: the data's total shared out and jittered
    x0[0] = 0.4 * total * (1.0 + 0.1 * x0[0])
    x0[1] = 0.6 * total * (1.0 + 0.1 * x0[1])
    assert eng.Start(x0)
    for when, steps in (("start", 0), ("accepted", 2)):
        if steps:
            eng.Step(steps)
        x, logl = eng.GetAccepted(), eng.lane("logl")
        assert logl.shape == (nchains,)
        for c in range(nchains):
            assert tref.same(logl[c], host(x[:, c])), "%s, chain %d" % (when, c)
        for c in (0, 1, 1024):
            assert tref.same(logl[c], tref.evaluate(params, x[:, c], be)[0]), "%s, chain %d: the restatement" % (when, c)
    assert not np.array_equal(x, x0)
    eng.close()
