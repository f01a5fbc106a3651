"""SMCMC_LIKE_EVENT_TEMPLATE restated in Python from the definition in include/smcmc.h (example2/ of the reference), for
the tests of the template-fit likelihood.  The per-event part -- corrected mass, scaled separation, cuts, split and bin
rule -- is SMCMC_LIKE_EVENT_SAMPLE's and is taken from tests/event_sample_ref.py (the `where` of its evaluate); the
weights, the six histograms, the class integrals, the normalisations, the expectation, the bin sum and the penalties are
written here, operation by operation in the definition's order.  Python's + - * / on floats are single IEEE
operations, un-fused.
"""
import importlib.util
import math
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_here, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("smcmc_event_sample_ref", "event_sample_ref.py")
cases = _load("smcmc_event_sample_cases", "event_sample_cases.py")


def weights(point, true_fakes, true_eff, be):
    """{(background, tagged): weight}: example2/SystematicCorrection.H:76-115 without WEIGHT_SIGNAL_ANYWAY"""
    p = [float(v) for v in point]
    cf = math.tan(math.pi * (true_fakes - 0.5))                # :93 (a constant of the sample, from libm)
    cf += p[7]                                                 # :94
    cf = be.atan1(cf) / math.pi + 0.5                          # :95
    ce = math.tan(math.pi * (true_eff - 0.5))                  # :105
    ce += p[8]                                                 # :106
    ce = be.atan1(ce) / math.pi + 0.5                          # :107
    return {(0, 1): cf / true_fakes,                           # :98
            (0, 0): (1.0 - cf) / (1.0 - true_fakes),           # :99
            (1, 1): ce / true_eff,                             # :110
            (1, 0): (1.0 - ce) / (1.0 - true_eff)}             # :111


def integral(hist, nbins):
    """step 2: the three sums over the bins ascending from +0, added DecayTag + Close, then + Separated"""
    sums = []
    for h in range(3):
        s = 0.0
        for b in range(nbins):
            s += hist[h * nbins + b]
        sums.append(s)
    v = sums[2]
    v += sums[0]
    v += sums[1]
    return v


def _div(a, b):
    """one IEEE division, as C has it: x / 0 is +-inf or NaN"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def _add(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) + np.float64(b))


def penalties(logl, p):
    """step 5"""
    if p[0] < 0.0:
        logl -= 10.0 + abs(logl)
    if p[1] < 0.0:
        logl -= 10.0 + abs(logl)
    v = p[6] / 5.0
    logl -= (0.5 * v) * v
    v = p[7] / 1.0
    logl -= (0.5 * v) * v
    v = p[8] / 1.0
    logl -= (0.5 * v) * v
    return logl


def evaluate(params, point, be):
    """-> (logL, mc[3 nbins] as a list, parts: {"S", "B": lists of 3 nbins, "IS", "IB", "ws", "wb"}, where[nevents])"""
    nev, nbins, xmin, xmax, exposure, cut, true_fakes, true_eff, data, ev = ref.split(params)
    p = [float(v) for v in point]
    _, _, where = ref.evaluate(params, point, be)              # the per-event part: LIKE 7's, unchanged
    w = weights(p, true_fakes, true_eff, be)
    S, B = [0.0] * (3 * nbins), [0.0] * (3 * nbins)
    for i in range(nev):                                       # step 1
        if where[i] < 0:
            continue
        background = 1 if ev[i, 1] > 0 else 0
        h = B if background else S
        h[where[i]] = h[where[i]] + w[(background, 1 if ev[i, 3] > 0 else 0)]
    IS, IB = integral(S, nbins), integral(B, nbins)            # step 2
    ws, wb = _div(p[0], IS), _div(p[1], IB)
    mc = [_add(_add(0.0, _mul(ws, S[k])), _mul(wb, B[k])) for k in range(3 * nbins)]    # step 3
    logl = 0.0
    for k in range(3 * nbins):                                 # step 4
        d = float(data[k])
        m = mc[k]
        if m < 0.001:
            m = 0.001
        v = d - m
        if d > 0.0:
            v += d * be.log1(_div(m, d))
        logl += v
    return penalties(logl, p), mc, {"S": S, "B": B, "IS": IS, "IB": IB, "ws": ws, "wb": wb}, where


def same(a, b):
    """bit for bit, NaN compared as NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def make_sample(oracle, nsignal, nbackground, nbins, key):
    """event_sample_ref.make_sample with the exposure ratio the template fit demands"""
    params = ref.make_sample(oracle, nsignal, nbackground, nbins, key)
    params[4] = 1.0
    return params


def keep_classes(params, nsignal, nbackground):
    """The first nsignal signal and the first nbackground background events of a sample, signal first: ref.truncate
    cannot choose the class counts."""
    params = np.asarray(params, dtype=np.float64)
    nev, nbins = int(params[0]), int(params[1])
    ev = params[8 + 3 * nbins:].reshape(nev, 6)
    sig, bkg = ev[ev[:, 1] <= 0], ev[ev[:, 1] > 0]
    assert 1 <= nsignal <= len(sig) and 1 <= nbackground <= len(bkg)
    out = np.concatenate([params[:8 + 3 * nbins], sig[:nsignal].ravel(), bkg[:nbackground].ravel()])
    out[0] = nsignal + nbackground
    return out


def interleave(params, seed):
    """the same events in a random order that keeps each class's own order (a random merge of the two classes)"""
    params = np.asarray(params, dtype=np.float64)
    nev, nbins = int(params[0]), int(params[1])
    ev = params[8 + 3 * nbins:].reshape(nev, 6)
    sig, bkg = list(ev[ev[:, 1] <= 0]), list(ev[ev[:, 1] > 0])
    take_signal = np.zeros(nev, dtype=bool)
    take_signal[np.random.default_rng(seed).choice(nev, len(sig), replace=False)] = True
    rows = [sig.pop(0) if t else bkg.pop(0) for t in take_signal]
    return np.concatenate([params[:8 + 3 * nbins], np.array(rows).ravel()])


def class_counts(params):
    nev, nbins = int(params[0]), int(params[1])
    types = np.asarray(params[8 + 3 * nbins:]).reshape(nev, 6)[:, 1]
    return int(np.sum(types <= 0)), int(np.sum(types > 0))


def points(oracle, n, key, params):
    """n points: ref.points' systematic parameters (the origin first, a mass skew beyond smcmc_erf's switch last), and
    for the two fitted counts the sample's own data total shared out, jittered -- except two points that keep ref.points'
    small values around zero, the first with a negative signal count, the second with a negative background count, where
    the sign penalties and the clamp of every bin are at work."""
    nbins = int(params[1])
    total = float(np.sum(params[8:8 + 3 * nbins]))
    pts = ref.points(oracle, n, key)
    for k, p in enumerate(pts):
        if n >= 4 and k in (n // 2, n // 2 + 1):
            p[k - n // 2] = -abs(p[k - n // 2])
            continue
        p[0] = 0.4 * total * (1.0 + 0.1 * p[0])
        p[1] = 0.6 * total * (1.0 + 0.1 * p[1])
    return pts
