"""SMCMC_LIKE_EVENT_TEMPLATE without a GPU: the host definition (smcmc_event_template_evaluate) against the restatement of
tests/event_template_ref.py bit for bit -- log-likelihood, expectation and every intermediate stage --, hand-counted
samples, the partition by class, the three rules the parameter array gains, the penalties and the two extreme points."""
import importlib.util
import math
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("smcmc_event_template_ref",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_template_ref.py"))
tref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tref)
ref, cases = tref.ref, tref.cases

ERR_INVALID = 1
CASES = [(60, 137, 50, 101), (30, 34, 5, 102)]    # signal, background (197 and 64 events), nbins, key


@pytest.fixture(scope="module", params=CASES, ids=["197ev_50bins", "64ev_5bins"])
def case(request, oracle, smcmc):
    nsig, nbkg, nbins, key = request.param
    params = tref.make_sample(oracle, nsig, nbkg, nbins, key)
    pts = tref.points(oracle, 12, key + 1000, params)
    be = ref.deterministic(oracle, smcmc)
    return params, pts, [tref.evaluate(params, p, be) for p in pts], be


def _check(smcmc, params, point, want):
    logl, mc, parts, _ = want
    got, hist, gp = smcmc.event_template_evaluate(params, point, histograms=True, parts=True)
    assert tref.same(gp["S"].ravel(), parts["S"]) and tref.same(gp["B"].ravel(), parts["B"])
    for k in ("IS", "IB", "ws", "wb"):
        assert tref.same(gp[k], parts[k]), k
    assert tref.same(hist.ravel(), mc)
    assert tref.same(got, logl)
    assert tref.same(smcmc.event_template_evaluate(params, point), logl)       # (without the optional outputs)


def test_host_definition_is_the_restatement_bit_for_bit(case, smcmc):
    params, pts, det, be = case
    assert len(pts) == 12
    for p, want in zip(pts, det):
        _check(smcmc, params, p, want)
        assert math.isfinite(want[0])
    # the points meet the branches: both signs of both counts, the clamp opposite data, bins of no data
    assert any(p[0] < 0 for p in pts) and any(p[1] < 0 for p in pts) and any(p[0] > 0 and p[1] > 0 for p in pts)
    data = ref.split(params)[8]
    assert any(m < 0.001 and d > 0 for want in det for m, d in zip(want[1], data)) and np.any(data == 0)


def test_hand_counted_one_signal_one_background_event(smcmc):
    """a signal event of mass 135 that is Close and a tagged background event of mass 320, five bins of 100: S holds one
    weight in Close bin 1, B one in DecayTag bin 3, each class integrates to its one weight and is scaled to its count"""
    nbins = 5
    data = np.arange(1.0, 16.0).reshape(3, nbins)
    events = np.array([[135.0, 0, 50.0, 0, 135.0, 40.5], [320.0, 2, 150.0, 1, 320.0, 96.0]])
    params = smcmc.event_sample_params(events, data, nbins, 0.0, 500.0, exposure_ratio=1.0)
    p = np.zeros(9)
    p[0], p[1] = 7.0, 11.0
    logl, hist, parts = smcmc.event_template_evaluate(params, p, histograms=True, parts=True)
    S, B = parts["S"].ravel(), parts["B"].ravel()
    assert list(np.flatnonzero(S)) == [1] and list(np.flatnonzero(B)) == [2 * nbins + 3]
    assert S[1] == pytest.approx(1.0, rel=1e-14) and B[13] == pytest.approx(1.0, rel=1e-14)      # (1 - cf) / 0.95, ce / 0.5
    assert parts["IS"] == S[1] and parts["IB"] == B[13]
    assert parts["ws"] == 7.0 / S[1] and parts["wb"] == 11.0 / B[13]
    want = np.zeros(3 * nbins)
    want[1], want[13] = parts["ws"] * S[1], parts["wb"] * B[13]
    assert np.array_equal(hist.ravel(), want)
    total = 0.0
    for k, d in enumerate(data.ravel()):
        mc = max(want[k], 0.001)
        total += d - mc + d * math.log(mc / d)
    assert logl == pytest.approx(total, rel=1e-13)
    # the same two events, background first: the bits of the sorted sample
    swapped = smcmc.event_sample_params(events[::-1], data, nbins, 0.0, 500.0, exposure_ratio=1.0)
    assert smcmc.event_template_evaluate(swapped, p) == logl


def test_interleaved_sample_gives_the_bits_of_the_sorted_one(case, smcmc):
    params, pts, det, be = case
    mixed = tref.interleave(params, 5)
    nsig = tref.class_counts(params)[0]
    types = mixed[8 + 3 * int(params[1]):].reshape(-1, 6)[:, 1]
    assert np.any(types[:nsig] > 0) and sorted(mixed) == sorted(params)       # really interleaved, the same events
    for p, want in zip(pts, det):
        _check(smcmc, mixed, p, want[:3] + (None,))


def test_the_three_new_parameter_rules(case, smcmc):
    params, pts, det, be = case
    nbins = int(params[1])
    ev0 = 8 + 3 * nbins

    def refused(prm, text):
        with pytest.raises(smcmc.SmcmcError) as e:
            smcmc.event_template_evaluate(prm, np.zeros(9))
        assert e.value.status == ERR_INVALID and text in str(e.value)

    prm = params.copy(); prm[4] = 1.0 + 2.0 ** -52
    refused(prm, "exposureRatio must be exactly 1")
    prm = params.copy(); prm[ev0 + 1::6] = 1.0
    refused(prm, "at least one event must be signal")
    prm = params.copy(); prm[ev0 + 1::6] = 0.0
    refused(prm, "at least one event must be background")
    refused(params[:-1], "exactly")                                    # LIKE_EVENT_SAMPLE's rules hold as they did
    smcmc.event_sample_evaluate(prm, np.zeros(9))                      # ... and LIKE_EVENT_SAMPLE takes what it took


def test_penalties(case, smcmc):
    params, pts, det, be = case
    base = pts[1]
    seen = {}
    for name, p0, p1 in (("none", 40.0, 60.0), ("signal", -40.0, 60.0), ("background", 40.0, -60.0), ("both", -40.0, -60.0),
                         ("zero", 0.0, 60.0)):
        p = base.copy()
        p[0], p[1] = p0, p1
        want = tref.evaluate(params, p, be)
        _check(smcmc, params, p, want)
        seen[name] = (p, want)
    # the sign penalties act on the bin sum, one after the other: undo the three Gaussian terms' order by recomputing
    for name in ("signal", "background", "both"):
        p, (logl, mc, parts, _) = seen[name]
        bins = 0.0
        data = ref.split(params)[8]
        for k in range(len(mc)):
            m = max(mc[k], 0.001) if mc[k] == mc[k] else mc[k]
            v = float(data[k]) - m
            if data[k] > 0:
                v += float(data[k]) * be.log1(m / float(data[k]))
            bins += v
        after = bins - (10.0 + abs(bins))
        if name == "both":
            after = after - (10.0 + abs(after))                                # on the logL just updated
            assert after != bins - 2.0 * (10.0 + abs(bins))                    # (the order matters)
        for v in (p[6] / 5.0, p[7] / 1.0, p[8] / 1.0):
            after -= (0.5 * v) * v
        assert after == logl
    # p[0] == 0: ws is 0, every bin with no background is clamped
    p, (logl, mc, parts, _) = seen["zero"]
    assert parts["ws"] == 0.0 and math.isfinite(logl)
    assert all(m == 0.0 for m, b in zip(mc, parts["B"]) if b == 0.0) and any(b == 0.0 for b in parts["B"])


def test_extreme_points(case, smcmc):
    params, pts, det, be = case
    up, down = cases.extreme_points()
    for p in (up, down):
        p[0], p[1] = 40.0, 60.0
    want = tref.evaluate(params, up, be)
    assert want[2]["IS"] == 0.0 and want[2]["IB"] == 0.0 and math.isnan(want[0])      # all dropped: 40 / 0, NaN
    _check(smcmc, params, up, want)
    assert math.isnan(smcmc.event_template_evaluate(params, up))
    want = tref.evaluate(params, down, be)
    nbins = int(params[1])
    assert math.isfinite(want[0]) and set(np.flatnonzero(want[1])) <= {0, nbins, 2 * nbins}    # all in the first bins
    _check(smcmc, params, down, want)
