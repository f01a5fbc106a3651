"""SMCMC_LIKE_EVENT_SHAPE without a GPU: the host definition (smcmc_event_shape_evaluate) against the restatement of
tests/event_shape_ref.py bit for bit -- log-likelihood, expectation and every intermediate stage but the inverted
kernels, which the restatement takes from the library --, a hand-counted sample, the partition by class, every rule of
the parameter array, the shape's branches and the two extreme points."""
import importlib.util
import math
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("smcmc_event_shape_ref",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_shape_ref.py"))
sref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sref)
ref = sref.ref
_spec = importlib.util.spec_from_file_location("smcmc_event_shape_cases",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_shape_cases.py"))
scases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(scases)

ERR_INVALID = 1
CASES = [(60, 137, 50, 201), (30, 34, 5, 202)]    # signal, background (197 and 64 events), nbins, key
FIELDS = ("IS", "IB", "ws", "wb", "penB", "penS")


@pytest.fixture(scope="module", params=CASES, ids=["197ev_50bins", "64ev_5bins"])
def case(request, oracle, smcmc):
    nsig, nbkg, nbins, key = request.param
    params = sref.make_sample(oracle, nsig, nbkg, nbins, key)
    pts = sref.points(oracle, 12, key + 1000, params)
    be = ref.deterministic(oracle, smcmc)
    _, parts = smcmc.event_shape_evaluate(params, np.zeros(31), parts=True)
    kinv = (parts["KinvB"], parts["KinvS"])
    return params, pts, [sref.evaluate(params, p, be, *kinv) for p in pts], be, kinv


def _check(smcmc, params, point, want):
    logl, mc, parts, _ = want
    got, hist, gp = smcmc.event_shape_evaluate(params, point, histograms=True, parts=True)
    assert sref.same(gp["S"].ravel(), parts["S"]) and sref.same(gp["B"].ravel(), parts["B"])
    for k in FIELDS:
        assert sref.same(gp[k], parts[k]), k
    assert sref.same(hist.ravel(), mc)
    assert sref.same(got, logl)
    assert sref.same(smcmc.event_shape_evaluate(params, point), logl)          # (without the optional outputs)


def test_likelihood_nine_exists(smcmc):
    assert smcmc.LIKE_EVENT_SHAPE == 9


def test_host_definition_is_the_restatement_bit_for_bit(case, smcmc):
    params, pts, det, be, kinv = case
    assert len(pts) == 12
    for p, want in zip(pts, det):
        _check(smcmc, params, p, want)
        assert math.isfinite(want[0])
    # the points meet the branches: the origin, both signs of both counts, the clamp opposite data, bins of no data
    assert not np.any(pts[0][2:])
    assert any(p[0] < 0 for p in pts) and any(p[1] < 0 for p in pts) and any(p[0] > 0 and p[1] > 0 for p in pts)
    data = sref.split(params)["data"]
    assert any(m < 0.001 and d > 0 for want in det for m, d in zip(want[1], data)) and np.any(data == 0)
    # ... every histogram is filled by both classes somewhere, and the penalties are at work
    S, B = np.array(det[1][2]["S"]).reshape(4, -1), np.array(det[1][2]["B"]).reshape(4, -1)
    assert np.all(S.sum(axis=1) > 0) and np.all(B.sum(axis=1) > 0)
    assert det[1][2]["penB"] > 0 and det[1][2]["penS"] > 0 and det[0][2]["penB"] == 0.0


def test_the_sample_covers_the_shape_rule(case):
    params = case[0]
    f = sref.split(params)
    y = [float(i + 1) for i in range(13)]
    seen = set()
    for row in f["ev"]:
        n, lo, hi = (sref.NB, f["bkg_low"], f["bkg_high"]) if row[1] > 0 else (sref.NS, f["sig_low"], f["sig_high"])
        c = sref.centres(lo, hi, n)
        _, k, clamped = sref.shape(float(row[0]), y[:n], lo, hi)
        x = float(row[0])
        kind = ("low" if k == 0 else "high") if clamped else ("centre" if x == c[k + 1] else "lower" if x - c[k] < 0.5 * (c[1] - c[0]) else "upper")
        seen.add((row[1] > 0, kind))
        if x > hi:
            seen.add((row[1] > 0, "beyond"))
    assert seen == {(b, k) for b in (False, True) for k in ("low", "high", "centre", "lower", "upper", "beyond")}


def test_hand_counted_one_signal_one_background_event(smcmc):
    """a signal event of mass 135 at separation 20 (VeryClose) and a tagged background event of mass 320, five bins of
    100; the shapes: signal control points 6 and 7 (centres 125 and 144.23...) set, background's all 0.5"""
    nbins = 5
    data = np.arange(1.0, 21.0).reshape(4, nbins)
    events = np.array([[135.0, 0, 20.0, 0, 135.0, 40.5], [320.0, 2, 150.0, 1, 320.0, 96.0]])
    params = smcmc.event_shape_params(events, data, nbins, 0.0, 500.0)
    p = np.zeros(31)
    p[0], p[1] = 7.0, 11.0
    p[9:20] = 5.0                       # yB = 0.5 everywhere: exp(0.5)
    p[20 + 5], p[20 + 6] = 2.0, 4.0     # yS[6] = 0.2 at 125, yS[7] = 0.4 at 144.23
    logl, hist, parts = smcmc.event_shape_evaluate(params, p, histograms=True, parts=True)
    S, B = parts["S"].ravel(), parts["B"].ravel()
    assert list(np.flatnonzero(S)) == [1] and list(np.flatnonzero(B)) == [3 * nbins + 3]
    cs = sref.centres(0.0, 250.0, 13)
    assert cs[6] == 125.0
    want_s = math.exp(0.2 + (135.0 - 125.0) * (0.4 - 0.2) / (cs[7] - cs[6]))
    assert S[1] == pytest.approx(want_s, rel=1e-13) and B[18] == pytest.approx(math.exp(0.5), rel=1e-13)
    assert parts["IS"] == S[1] and parts["IB"] == B[18]
    assert parts["ws"] == 7.0 / S[1] and parts["wb"] == 11.0 / B[18]
    want = np.zeros(4 * nbins)
    want[1], want[18] = parts["ws"] * S[1], parts["wb"] * B[18]
    assert np.array_equal(hist.ravel(), want)
    yb, ys = sref.control_values(list(p))
    assert parts["penB"] == pytest.approx(float(np.array(yb) @ np.linalg.inv(sref.split(params)["KB"]) @ np.array(yb)), rel=1e-6)
    assert parts["penS"] == pytest.approx(float(np.array(ys) @ np.linalg.inv(sref.split(params)["KS"]) @ np.array(ys)), rel=1e-4)
    total = 0.0
    for k, d in enumerate(data.ravel()):
        mc = max(want[k], 0.001)
        total += d - mc + d * math.log(mc / d)
    assert logl == pytest.approx(total - parts["penB"] - parts["penS"], rel=1e-12)
    swapped = smcmc.event_shape_params(events[::-1], data, nbins, 0.0, 500.0)
    assert smcmc.event_shape_evaluate(swapped, p) == logl


def test_interleaved_sample_gives_the_bits_of_the_sorted_one(case, smcmc):
    params, pts, det, be, kinv = case
    sorted_params = np.concatenate([params[:sref.events_offset(params)],
                                    sref.keep_classes(params, *_counts(params))[sref.events_offset(params):]])
    mixed = sref.interleave(params, 5)
    nsig = _counts(params)[0]
    types = mixed[sref.events_offset(params):].reshape(-1, 6)[:, 1]
    assert np.any(types[:nsig] > 0) and sorted(mixed) == sorted(params)       # really interleaved, the same events
    for p, want in zip(pts, det):
        _check(smcmc, mixed, p, want[:3] + (None,))
        _check(smcmc, sorted_params, p, want[:3] + (None,))


def _counts(params):
    types = sref.split(params)["ev"][:, 1]
    return int(np.sum(types <= 0)), int(np.sum(types > 0))


def test_every_parameter_rule(case, smcmc):
    params, pts, det, be, kinv = case
    nbins = int(params[1])
    kb0 = sref.HEAD + 4 * nbins
    ks0 = kb0 + 121
    ev0 = sref.events_offset(params)

    def refused(prm, text):
        with pytest.raises(smcmc.SmcmcError) as e:
            smcmc.event_shape_evaluate(prm, np.zeros(31))
        assert e.value.status == ERR_INVALID and text in str(e.value), str(e.value)

    def with_(index, value):
        prm = params.copy()
        prm[index] = value
        return prm

    refused(params[:-1], "exactly")
    refused(np.concatenate([params, [0.0]]), "exactly")
    refused(params[:5], "EVENT_SHAPE needs")
    refused(with_(3, math.inf), "header field is not finite")
    refused(with_(1, 0.0), "nbins")
    refused(with_(1, nbins + 0.5), "nbins")
    refused(with_(1, smcmc._capi.EVENT_SHAPE_MAX_BINS + 1.0), "nbins")
    refused(with_(0, 0.0), "nevents")
    refused(with_(2, params[3]), "xmin must be below xmax")
    refused(with_(4, params[5] + 1.0), "cutVeryClose must not be above cutClose")
    smcmc.event_shape_evaluate(with_(4, params[5]), np.zeros(31))              # (equal cuts: Close is empty, allowed)
    refused(with_(6, 0.0), "inside (0, 1)")
    refused(with_(7, 1.0), "inside (0, 1)")
    refused(with_(8, params[9]), "bkgLow must be below bkgHigh")
    refused(with_(10, params[11] + 1.0), "sigLow must be below sigHigh")
    refused(with_(sref.HEAD + 2, math.nan), "not finite")
    refused(with_(kb0 + 5, math.inf), "not finite")
    refused(with_(ev0 + 0, 0.0), "must be > 0")
    refused(with_(ev0 + 4, -1.0), "must be > 0")
    refused(with_(ev0 + 5, 0.0), "must be > 0")
    refused(with_(ev0 + 1, -1.0), "Type must be")
    prm = params.copy(); prm[ev0 + 1::6] = 1.0
    refused(prm, "at least one event must be signal")
    prm = params.copy(); prm[ev0 + 1::6] = 0.0
    refused(prm, "at least one event must be background")
    refused(with_(kb0 + 1, np.nextafter(params[kb0 + 1], 1.0)), "background's kernel is not symmetric")
    refused(with_(ks0 + 13, np.nextafter(params[ks0 + 13], 1.0)), "signal's kernel is not symmetric")
    prm = params.copy(); prm[kb0:kb0 + 121] = 1.0                              # rank one: a zero pivot
    refused(prm, "background's kernel cannot be inverted")
    prm = params.copy(); prm[ks0:ks0 + 169] = 0.0
    refused(prm, "signal's kernel cannot be inverted")
    with pytest.raises(smcmc.SmcmcError):
        smcmc.event_shape_evaluate(params, np.zeros(9))


def test_penalties(case, smcmc):
    params, pts, det, be, kinv = case
    base = pts[1]
    for p0, p1 in ((40.0, 60.0), (-40.0, 60.0), (40.0, -60.0), (-40.0, -60.0), (0.0, 60.0)):
        p = base.copy()
        p[0], p[1] = p0, p1
        want = sref.evaluate(params, p, be, *kinv)
        _check(smcmc, params, p, want)
        if p0 == 0.0:
            assert want[2]["ws"] == 0.0 and math.isfinite(want[0])
    # the signal's fixed zeros are in the penalty's sum and change nothing; the penalty is what numpy makes of it
    yb, ys = sref.control_values([float(v) for v in base])
    assert ys[0] == 0.0 and ys[12] == 0.0
    assert det[1][2]["penS"] == pytest.approx(float(np.array(ys) @ np.asarray(kinv[1]) @ np.array(ys)), rel=1e-9)
    assert det[1][2]["penB"] == pytest.approx(float(np.array(yb) @ np.asarray(kinv[0]) @ np.array(yb)), rel=1e-9)


def test_extreme_points(case, smcmc):
    params, pts, det, be, kinv = case
    up, down = sref.extreme_points(params)
    want = sref.evaluate(params, up, be, *kinv)
    assert want[2]["IS"] == 0.0 and want[2]["IB"] == 0.0 and math.isnan(want[0])      # all dropped: count / 0, NaN
    _check(smcmc, params, up, want)
    assert math.isnan(smcmc.event_shape_evaluate(params, up))
    want = sref.evaluate(params, down, be, *kinv)
    nbins = int(params[1])
    assert math.isfinite(want[0]) and set(np.flatnonzero(want[1])) <= {0, nbins, 2 * nbins, 3 * nbins}
    _check(smcmc, params, down, want)


def test_python_kernel_is_the_restatements(smcmc):
    kb, ks = sref.example3_kernels()
    assert np.array_equal(smcmc.event_shape_kernel(0.0, 500.0, 11, 100.0, 0.7), kb)
    assert np.array_equal(smcmc.event_shape_kernel(0.0, 250.0, 13, 50.0), ks)
    far = smcmc.event_shape_kernel(0.0, 500.0, 11, 5.0)
    assert far[0, 10] == 0.0 and far[0, 1] == 0.0 and far[0, 0] == 1.0        # r > 20 -> exactly 0
    ex = smcmc.event_shape_kernel(0.0, 500.0, 11, 100.0, 2.0, exponential=True)
    assert ex[0, 1] == pytest.approx(4.0 * math.exp(-(500.0 / 11) / 100.0), rel=1e-15)


def test_device_samples_are_what_they_are_meant_to_be(oracle, smcmc):
    """the samples of the device tests (tests/event_shape_cases.py): the class counts, the separations on the cuts, the shape's branches in the binned samples"""
    for kernel, all_counts in (("ensemble", scases.ENSEMBLE_COUNTS), ("per_chain", scases.PER_CHAIN_COUNTS)):
        for counts in all_counts:
            types = sref.split(scases.counted(oracle, kernel, *counts))["ev"][:, 1]
            assert (int(np.sum(types <= 0)), int(np.sum(types > 0))) == counts
    for spec in list(scases.ENSEMBLE_BINS.values()) + list(scases.PER_CHAIN_BINS.values()):
        f = sref.split(scases.with_separations_on_the_cuts(scases.binned(oracle, spec)))
        assert f["nbins"] <= scases.MAX_BINS == smcmc._capi.EVENT_SHAPE_MAX_BINS
        sig_masses, bkg_masses = sref.shape_masses()
        for background, masses in ((False, sig_masses), (True, bkg_masses)):
            rows = f["ev"][(f["ev"][:, 1] > 0) == background]
            assert set(masses) <= set(rows[:, 0])
            assert 50.0 in rows[rows[:, 3] == 0][:, 2] and 100.0 in rows[rows[:, 3] == 0][:, 2]
    owners = sorted({(4 * spec[2] + 63) // 64 for spec in scases.PER_CHAIN_BINS.values()})
    assert owners == [1, 2, 3, 4]                          # every count of owner registers
