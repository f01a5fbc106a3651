"""The posterior-predictive histograms of a saved trace (smcmc_event_predictive_sums, include/smcmc.h), the host's side:
the result class PosteriorPredictive from sums made by hand of the host evaluators' histograms, and what the entry point
refuses before it looks for a device.  tests/test_gpu_event_predictive.py has the device's side."""
import ctypes as C
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
tcases, scases = _load("event_template_cases"), _load("event_shape_cases")
tref, sref = tcases.tref, scases.sref
DP = C.POINTER(C.c_double)


def _member(smcmc, oracle, member):
    """(likelihood, params, header, names, the stacked host histograms [12][NH][nbins] at the sample's own points)"""
    if member == "sample":
        params = cases.sample(ref, oracle, "197ev_50bins")
        pts = cases.points(ref, oracle, "197ev_50bins")
        like, header, evaluate, names = smcmc.LIKE_EVENT_SAMPLE, 8, smcmc.event_sample_evaluate, ("Close", "Separated", "DecayTag")
    elif member == "template":
        params = tcases.light_background_first(tref.make_sample(oracle, 30, 34, 5, 102))
        pts = tref.points(oracle, 12, 1102, params)
        like, header, evaluate, names = smcmc.LIKE_EVENT_TEMPLATE, 8, smcmc.event_template_evaluate, ("Close", "Separated", "DecayTag")
    else:
        params = sref.light_background_first(sref.make_sample(oracle, 30, 34, 5, 202))
        pts = sref.points(oracle, 12, 1202, params)
        like, header, evaluate = smcmc.LIKE_EVENT_SHAPE, 12, smcmc.event_shape_evaluate
        names = ("VeryClose", "Close", "Separated", "DecayTag")
    assert len(pts) == 12
    hists = np.array([evaluate(params, p, histograms=True)[1] for p in pts])
    return like, params, header, names, hists


def _sums(hists, centre):
    y = hists - centre
    return y.sum(axis=0), (y * y).sum(axis=0)


@pytest.mark.parametrize("member", ["sample", "template", "shape"])
def test_posterior_predictive_from_host_made_sums(smcmc, oracle, member):
    """The twelve points as a trace of 2 slots x 6 chains: mean and spread per bin are numpy's of the stacked histograms,
    whether the sums are taken about the origin or about the mean; the halves of the chains, taken about different centres,
    add to the whole."""
    like, params, header, names, hists = _member(smcmc, oracle, member)
    nh, nbins = hists.shape[1:]
    assert nh == len(names) and nbins == int(params[1]) and np.all(np.isfinite(hists))
    data = params[header:header + nh * nbins].reshape(nh, nbins)
    want_mean, want_spread = np.mean(hists, axis=0), np.std(hists, axis=0)
    assert np.any(want_spread > 0)
    for centre in (None, want_mean):
        s, q = _sums(hists, 0.0 if centre is None else centre)
        pp = smcmc.PosteriorPredictive(s.ravel(), q.ravel(), 2, 6, data, None if centre is None else centre.ravel())
        assert pp.names == names and pp.n == 12 and pp.nslots == 2 and pp.nchains == 6
        assert np.array_equal(pp.data, data) and pp.sum.shape == pp.sumsq.shape == pp.centre.shape == (nh, nbins)
        np.testing.assert_allclose(pp.mean, want_mean, rtol=1e-12, atol=0)
        np.testing.assert_allclose(pp.spread, want_spread, rtol=1e-12, atol=0)
        about = pp.about(want_mean + 0.25)
        np.testing.assert_allclose(about.mean, want_mean, rtol=1e-12, atol=0)
        assert np.array_equal(about.centre, want_mean + 0.25) and about.n == 12
    # points k = 6 slot + chain: chains 0 .. 2 about the origin, chains 3 .. 5 about another centre
    by_chain = hists.reshape(2, 6, nh, nbins)
    left = smcmc.PosteriorPredictive(*_sums(by_chain[:, :3].reshape(6, nh, nbins), 0.0), 2, 3, data)
    other = want_mean * 0.5 + 1.0
    right = smcmc.PosteriorPredictive(*_sums(by_chain[:, 3:].reshape(6, nh, nbins), other), 2, 3, data, other)
    whole = left + right
    assert whole.nchains == 6 and whole.nslots == 2 and whole.n == 12 and np.array_equal(whole.centre, left.centre)
    np.testing.assert_allclose(whole.mean, want_mean, rtol=1e-12, atol=0)
    np.testing.assert_allclose(whole.spread, want_spread, rtol=1e-12, atol=0)
    # what does not fit together
    s, q = _sums(hists, 0.0)
    with pytest.raises(ValueError):
        smcmc.PosteriorPredictive(s.ravel()[:-1], q.ravel()[:-1], 2, 6, data)
    with pytest.raises(ValueError):
        smcmc.PosteriorPredictive(s, q, 2, 6, data, np.zeros(nh * nbins + 1))
    with pytest.raises(ValueError):
        smcmc.PosteriorPredictive(s, q, 2, 6, data.ravel())
    with pytest.raises(ValueError):
        left + smcmc.PosteriorPredictive(s, q, 3, 6, data)                      # another number of slots
    with pytest.raises(ValueError):
        left + smcmc.PosteriorPredictive(s[:, :-1], q[:, :-1], 2, 6, data[:, :-1])  # another number of bins
    with pytest.raises(ValueError):
        left.about(np.zeros(nh * nbins + 1))


def _call(lib, like, params, count, trace=64, nslots=2, dim_stride=9, nchains=3, npad=64, give_sum=True):
    """smcmc_event_predictive_sums with a trace pointer nothing may dereference; (status, sum, sumsq)"""
    rows = 4 * 97
    s, q = np.full(rows, -7.0), np.full(rows, -7.0)
    st = lib.smcmc_event_predictive_sums(like, params.ctypes.data_as(DP), count, C.c_void_p(trace), nslots, dim_stride, nchains,
                                         npad, None, None, None, s.ctypes.data_as(DP) if give_sum else None,
                                         q.ctypes.data_as(DP), None)
    return st, s, q


def test_entry_point_refusals_need_no_device(smcmc, oracle):
    """Every refusal is SMCMC_ERR_INVALID (1) before a device is looked for, with nothing written; a broken parameter rule
    leaves its text for smcmc_event_sample_last_error.  A well-formed call without a device is SMCMC_ERR_NO_DEVICE (7)."""
    lib = smcmc.load()
    es = np.ascontiguousarray(cases.sample(ref, oracle, "5ev_5bins"))
    et = np.ascontiguousarray(tcases.counted(oracle, "ensemble", 4, 4))
    esh = np.ascontiguousarray(scases.counted(oracle, "ensemble", 4, 4))
    E, T, S = smcmc.LIKE_EVENT_SAMPLE, smcmc.LIKE_EVENT_TEMPLATE, smcmc.LIKE_EVENT_SHAPE
    assert (E, T, S) == (7, 8, 9)

    def refused(st, s, q):
        return st == 1 and np.all(s == -7.0) and np.all(q == -7.0)

    def text():
        return lib.smcmc_event_sample_last_error().decode()

    assert refused(*_call(lib, 0, es, es.size))
    assert refused(*_call(lib, 10, es, es.size))
    assert refused(*_call(lib, E, es, es.size - 1)) and "exactly" in text()
    half = et.copy()
    half[4] = 0.5
    assert refused(*_call(lib, T, half, half.size)) and "exposureRatio" in text()
    assert refused(*_call(lib, E, es, es.size, dim_stride=8))
    assert refused(*_call(lib, S, esh, esh.size, dim_stride=30))
    assert refused(*_call(lib, E, es, es.size, npad=65))
    assert refused(*_call(lib, E, es, es.size, nslots=0))
    assert refused(*_call(lib, E, es, es.size, give_sum=False))
    assert refused(*_call(lib, E, es, es.size, trace=0))
    import torch
    if torch.cuda.is_available():
        return                           # tests/test_gpu_event_predictive.py has the device's side
    for like, prm, stride in ((E, es, 9), (T, et, 15), (S, esh, 31)):
        st, s, q = _call(lib, like, prm, prm.size, dim_stride=stride)
        assert st == 7 and np.all(s == -7.0) and np.all(q == -7.0)
        assert text() == ""
    with pytest.raises(smcmc.SmcmcError) as err:
        smcmc.event_predictive(E, es, 64, 2, 9, 3, 64)
    assert err.value.status == 7
    with pytest.raises(smcmc.SmcmcError) as err:
        smcmc.event_predictive(T, half, 64, 2, 9, 3, 64)
    assert err.value.status == 1 and "exposureRatio" in str(err.value)
