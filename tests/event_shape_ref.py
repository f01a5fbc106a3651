"""SMCMC_LIKE_EVENT_SHAPE restated in Python from the definition in include/smcmc.h (example3/ of the reference with
TFakeGP.H), for the tests of the likelihood with Gaussian-process shape weights.  Everything is written here, operation by
operation in the definition's order, on the backends of tests/event_sample_ref.py (the deterministic elementary
functions of the oracle and the library, or libm's).  Python's + - * / on floats are single IEEE operations, un-fused.
The inverted kernels are an input (the library's own, from the `parts` of smcmc_event_shape_evaluate): how good that
inverse is, tests/test_event_shape_truth_cpu.py measures against mpmath.
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

HEAD = 12
NB, NS = 11, 13
HISTS = ("VeryClose", "Close", "Separated", "DecayTag")


def split(params):
    """dict of the array's fields (include/smcmc.h)"""
    params = np.asarray(params, dtype=np.float64)
    nev, nbins = int(params[0]), int(params[1])
    names = ("xmin", "xmax", "cut_very_close", "cut_close", "true_fakes", "true_eff", "bkg_low", "bkg_high", "sig_low", "sig_high")
    out = {k: float(v) for k, v in zip(names, params[2:HEAD])}
    at = HEAD
    out.update(nev=nev, nbins=nbins, data=params[at:at + 4 * nbins])
    at += 4 * nbins
    out["KB"] = params[at:at + 121].reshape(NB, NB)
    out["KS"] = params[at + 121:at + 290].reshape(NS, NS)
    out["ev"] = params[at + 290:].reshape(nev, 6)
    return out


def events_offset(params):
    return HEAD + 4 * int(params[1]) + 290


def centres(low, high, n):
    bw = (high - low) / n
    return [low + i * bw + 0.5 * bw for i in range(n)]


def control_values(p):
    """(yB[11], yS[13]): example3/SystematicCorrection.H:136-149"""
    yb = [p[9 + i] / 10.0 for i in range(NB)]
    ys = [0.0] * NS
    for i in range(11):
        ys[i + 1] = p[20 + i] / 10.0
    return yb, ys


def _div(a, b):
    """one IEEE division, as C has it: x / 0 is +-inf or NaN"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _mul(a, b):
    """(Python's float * + - never raise: inf and NaN come out as IEEE has them)"""
    return a * b


def _add(a, b):
    return a + b


def _sub(a, b):
    return a - b


def shape(x, y, low, high):
    """TFakeGP::GetValue = TH1::Interpolate as smcmc.h states it; -> (value, k, clamped)"""
    n = len(y)
    c = centres(low, high, n)
    if x <= c[0]:
        return y[0], 0, True
    if x >= c[n - 1]:
        return y[n - 1], n - 1, True
    b = int((float(n) * (x - low)) / (high - low))
    k = b - 1 if x <= c[b] else b
    slope = _div(_sub(y[k + 1], y[k]), c[k + 1] - c[k])
    return _add(y[k], _mul(x - c[k], slope)), k, False


def gp_penalty(y, kinv):
    """TFakeGP::GetPenalty, TFakeGP.H:137-145"""
    pen = 0.0
    for i in range(len(y)):
        for j in range(len(y)):
            pen = _add(pen, _mul(_mul(y[i], y[j]), float(kinv[i][j])))
    return pen


def integral(hist, nbins):
    """the four sums over the bins ascending from +0, added DecayTag + VeryClose + Close + Separated"""
    sums = []
    for h in range(4):
        s = 0.0
        for b in range(nbins):
            s = _add(s, hist[h * nbins + b])
        sums.append(s)
    v = sums[3]
    v = _add(v, sums[0])
    v = _add(v, sums[1])
    v = _add(v, sums[2])
    return v


def penalties(logl, p, pen_b, pen_s):
    if p[0] < 0.0:
        logl = _sub(logl, _add(10.0, abs(logl)))
    if p[1] < 0.0:
        logl = _sub(logl, _add(10.0, abs(logl)))
    for v in (p[3] / 5.0, p[4] / 1.0, p[5] / 1.0):
        logl = _sub(logl, _mul(_mul(0.5, v), v))
    logl = _sub(logl, pen_b)
    logl = _sub(logl, pen_s)
    return logl


def evaluate(params, point, be, kinv_b, kinv_s):
    """-> (logL, mc[4 nbins] as a list, parts: {"S", "B": lists of 4 nbins, "IS", "IB", "ws", "wb", "penB", "penS"},
    where[nevents]: the flat bin an event was filled into, or -1 mass > 500, -2 mass < 0, -3 separation < 0, -4 outside
    the axis)"""
    f = split(params)
    nev, nbins, ev = f["nev"], f["nbins"], f["ev"]
    p = [float(v) for v in point]
    assert len(p) == 31
    Mass, Type, Sep, MuDk, TrueMass, TrueSigma = (np.ascontiguousarray(ev[:, k]) for k in range(6))
    with np.errstate(all="ignore"):
        # example3/SystematicCorrection.H:48-76, InvariantMass
        nominalLogMass = be.log(TrueMass)
        nominalLogSigma = be.log(TrueMass + TrueSigma)
        nominalLogSigma = nominalLogSigma - nominalLogMass
        logMass = be.log(Mass)
        logSigma = (logMass - nominalLogMass) / nominalLogSigma
        scale = p[6] / 10.0
        width = be.exp1(p[7] / 10.0)
        skew = 0.3 * be.erf1(p[8] / 10.0)
        skewv = be.exp(logSigma * skew)
        logMass = nominalLogMass + (logMass - nominalLogMass) * skewv
        logMass = nominalLogMass + (logMass - nominalLogMass) * width
        logMass = logMass + scale
        mass = be.exp(logMass)
        # :34-46, Separation
        sep_scale = (be.exp1(p[2] / 10.0), be.exp1(p[3] / 10.0))
        sep = Sep * np.where(Type > 0, sep_scale[1], sep_scale[0])
    # :78-124, EventWeight
    cf = math.tan(math.pi * (f["true_fakes"] - 0.5))
    cf += p[4] / 10.0
    cf = be.atan1(cf) / math.pi + 0.5
    ce = math.tan(math.pi * (f["true_eff"] - 0.5))
    ce += p[5] / 10.0
    ce = be.atan1(ce) / math.pi + 0.5
    weight = {(0, 1): cf / f["true_fakes"], (0, 0): (1.0 - cf) / (1.0 - f["true_fakes"]),
              (1, 1): ce / f["true_eff"], (1, 0): (1.0 - ce) / (1.0 - f["true_eff"])}
    yb, ys = control_values(p)
    S, B = [0.0] * (4 * nbins), [0.0] * (4 * nbins)
    where = [0] * nev
    for i in range(nev):
        m, s = float(mass[i]), float(sep[i])
        background = 1 if Type[i] > 0 else 0
        if background:
            sh, _, _ = shape(float(Mass[i]), yb, f["bkg_low"], f["bkg_high"])
        else:
            sh, _, _ = shape(float(Mass[i]), ys, f["sig_low"], f["sig_high"])
        w = _mul(weight[(background, 1 if MuDk[i] > 0 else 0)], be.exp1(sh))
        if m > 500.0:
            where[i] = -1
            continue
        if m < 0.0:
            where[i] = -2
            continue
        if s < 0.0:
            where[i] = -3
            continue
        if MuDk[i] > 0:
            h = 3
        elif s < f["cut_very_close"]:
            h = 0
        elif s < f["cut_close"]:
            h = 1
        else:
            h = 2
        if not (m >= f["xmin"]) or not (m < f["xmax"]):
            where[i] = -4
            continue
        b = int((float(nbins) * (m - f["xmin"])) / (f["xmax"] - f["xmin"]))
        if b > nbins - 1:
            b = nbins - 1
        hh = B if background else S
        hh[h * nbins + b] = _add(hh[h * nbins + b], w)
        where[i] = h * nbins + b
    IS, IB = integral(S, nbins), integral(B, nbins)
    ws, wb = _div(p[0], IS), _div(p[1], IB)
    mc = [_add(_add(0.0, _mul(ws, S[k])), _mul(wb, B[k])) for k in range(4 * nbins)]
    logl = 0.0
    for k in range(4 * nbins):
        d = float(f["data"][k])
        m = mc[k]
        if m < 0.001:
            m = 0.001
        v = _sub(d, m)
        if d > 0.0:
            v = _add(v, _mul(d, be.log1(_div(m, d))))
        logl = _add(logl, v)
    pen_b, pen_s = gp_penalty(yb, kinv_b), gp_penalty(ys, kinv_s)
    parts = {"S": S, "B": B, "IS": IS, "IB": IB, "ws": ws, "wb": wb, "penB": pen_b, "penS": pen_s}
    return penalties(logl, p, pen_b, pen_s), mc, parts, where


def same(a, b):
    """bit for bit, NaN compared as NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---- samples -----------------------------------------------------------------------------------------------------
def gaussian_kernel(low, high, n, coherence, sigma=1.0):
    """TFakeGP::GaussianKernel, TFakeGP.H:96-109"""
    c = centres(low, high, n)
    k = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            r = (c[i] - c[j]) / coherence
            r = 0.5 * r * r
            k[i, j] = k[j, i] = 0.0 if r > 20 else sigma * sigma * math.exp(-r)
    return k


def example3_kernels():
    """example3/SystematicCorrection.H:151-163"""
    return gaussian_kernel(0.0, 500.0, NB, 100.0, 0.7), gaussian_kernel(0.0, 250.0, NS, 50.0, 1.0)


def assemble(ev, data, nbins, xmin=0.0, xmax=500.0, cuts=(50.0, 100.0), kernels=None):
    kb, ks = kernels if kernels is not None else example3_kernels()
    ev = np.asarray(ev, dtype=np.float64).reshape(-1, 6)
    head = [ev.shape[0], nbins, xmin, xmax, cuts[0], cuts[1], 0.05, 0.5, 0.0, 500.0, 0.0, 250.0]
    return np.concatenate([np.array(head, dtype=np.float64), np.asarray(data, dtype=np.float64).ravel(),
                           np.asarray(kb).ravel(), np.asarray(ks).ravel(), ev.ravel()])


def shape_masses(on_centres=True):
    """(signal masses, background masses) that cover every branch of the shape's rule: at or below the first centre and
    at or above the last centre of each shape, exactly on an interior centre, in the lower and in the upper half of a
    control bin, a signal mass above 250 and a background mass above 500"""
    cs, cb = centres(0.0, 250.0, NS), centres(0.0, 500.0, NB)
    off = 0.0 if on_centres else 0.37      # (off the centres, for a comparison with real arithmetic: a centre is rounded)
    sig = [cs[0] - off, 0.5 * cs[0], cs[NS - 1] + off, cs[5] + off, cs[4] - 3.0, cs[4] + 3.0, 251.5, 262.0]
    bkg = [cb[0] - off, 0.25 * cb[0], cb[NB - 1] + off, cb[3] + off, cb[6] - 9.0, cb[6] + 9.0, 499.0, 512.5]
    return sig, bkg


def make_sample(oracle, nsignal, nbackground, nbins, key, xmin=0.0, xmax=500.0, on_centres=True):
    """event_sample_ref.make_sample's events (a separation exactly 100, a background event far above xmax, both tags in
    both classes) under example3's header, kernels and four data histograms; and by construction a signal event whose
    separation is exactly 50, a Separated background event, and the masses of shape_masses() in the events that follow the constructed ones, as far as
    the class has room (TrueMass = Mass there, so that the origin leaves the mass where it is)."""
    base = ref.make_sample(oracle, nsignal, nbackground, nbins, key, xmin, xmax)
    ev = base[8 + 3 * nbins:].reshape(-1, 6).copy()
    if nsignal > 2:
        ev[2, 2], ev[2, 3] = 50.0, 0           # exactly cutVeryClose, untagged: Close
    if nbackground > 2:
        ev[nsignal + 2, 2], ev[nsignal + 2, 3] = 150.0, 0      # an untagged background event that is Separated
        ev[nsignal + 2, 0], ev[nsignal + 2, 4], ev[nsignal + 2, 5] = 213.7, 213.7, 64.0   # (on no bin edge)
    sig, bkg = shape_masses(on_centres)
    for k, m in enumerate(sig):
        if 3 + k < nsignal:
            ev[3 + k, 0], ev[3 + k, 4], ev[3 + k, 5] = m, m, 0.3 * m
    for k, m in enumerate(bkg):
        if 3 + k < nbackground:
            i = nsignal + 3 + k
            ev[i, 0], ev[i, 4], ev[i, 5] = m, m, 0.3 * m
    data = np.array([[1 + (7 * h + 3 * b) % 23 for b in range(nbins)] for h in range(4)], dtype=np.float64)
    data[0, 1 % nbins] = 0.0
    data[3, nbins - 1] = 0.0
    return assemble(ev, data, nbins, xmin, xmax)


def keep_classes(params, nsignal, nbackground):
    """the first nsignal signal and the first nbackground background events of a sample, signal first"""
    params = np.asarray(params, dtype=np.float64)
    at = events_offset(params)
    ev = params[at:].reshape(-1, 6)
    sig, bkg = ev[ev[:, 1] <= 0], ev[ev[:, 1] > 0]
    assert 1 <= nsignal <= len(sig) and 1 <= nbackground <= len(bkg)
    out = np.concatenate([params[:at], sig[:nsignal].ravel(), bkg[:nbackground].ravel()])
    out[0] = nsignal + nbackground
    return out


def light_background_first(params):
    """the same sample with the background events of Mass < 300 ahead of the other background events (a class none of
    whose first events survives has no finite likelihood to start a chain from)"""
    params = np.asarray(params, dtype=np.float64)
    at = events_offset(params)
    ev = params[at:].reshape(-1, 6)
    sig, bkg = ev[ev[:, 1] <= 0], ev[ev[:, 1] > 0]
    light = bkg[:, 0] < 300.0
    return np.concatenate([params[:at], sig.ravel(), bkg[light].ravel(), bkg[~light].ravel()])


def interleave(params, seed):
    """the same events in a random order that keeps each class's own order"""
    params = np.asarray(params, dtype=np.float64)
    at = events_offset(params)
    ev = params[at:].reshape(-1, 6)
    nev = len(ev)
    sig, bkg = list(ev[ev[:, 1] <= 0]), list(ev[ev[:, 1] > 0])
    take_signal = np.zeros(nev, dtype=bool)
    take_signal[np.random.default_rng(seed).choice(nev, len(sig), replace=False)] = True
    rows = [sig.pop(0) if t else bkg.pop(0) for t in take_signal]
    return np.concatenate([params[:at], np.array(rows).ravel()])


def data_total(params):
    nbins = int(params[1])
    return float(np.sum(params[HEAD:HEAD + 4 * nbins]))


def points(oracle, n, key, params, spread=3.0):
    """n points of 31 coordinates: the origin of the systematic and shape parameters first; then uniform in (-spread,
    spread), the last with a mass skew beyond the switch of smcmc_erf's two forms; the two counts the sample's data total
    shared out and jittered -- except two points that keep small values around zero, the first with a negative signal
    count, the second with a negative background count."""
    r = ref._Stream(oracle, key)
    total = data_total(params)
    pts = [np.zeros(31)]
    for k in range(1, n):
        pts.append(np.array([spread * (2.0 * r.uniform() - 1.0) for _ in range(31)]))
    pts[-1][8] = 12.0
    for k, p in enumerate(pts):
        if n >= 4 and k in (n // 2, n // 2 + 1):
            p[k - n // 2] = -abs(p[k - n // 2])
            continue
        p[0] = 0.4 * total * (1.0 + 0.1 * p[0])
        p[1] = 0.6 * total * (1.0 + 0.1 * p[1])
    return pts


def extreme_points(params):
    """(up, down): a mass scale that drops every event (every mass far above 500: both integrals 0, NaN) and one that
    puts every event into the first bins; the counts the sample's data total shared out"""
    total = data_total(params)
    up, down = np.zeros(31), np.zeros(31)
    up[6], down[6] = 100.0, -60.0
    for p in (up, down):
        p[0], p[1] = 0.4 * total, 0.6 * total
    return up, down
