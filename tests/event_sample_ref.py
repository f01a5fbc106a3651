"""SMCMC_LIKE_EVENT_SAMPLE restated in numpy / Python from the reference's lines, in the reference's order
(example/SystematicCorrection.H, example/FakeLikelihood.H), for the tests of the event-sample likelihood.

Two backends for the elementary functions:
  * deterministic(oracle, smcmc): oracle.det_exp / oracle.det_log and the library's host erf / atan
    (smcmc_selftest_detmath kinds 10, 11 with device = -1) -- what host and device must equal bit for bit;
  * libm(): math.exp, math.log, math.erf, math.atan -- the truth the deterministic functions stay close to.
numpy's elementwise + - * / on float64 are single IEEE operations, un-fused, so the per-event lines are written on
arrays; the Fill loop and the bin sum run event by event and bin by bin as the reference's loops do.

The samples are drawn here, deterministically, from oracle.philox with the distributions of example/Simulated.H.
"""
import math

import numpy as np


class Backend:
    def __init__(self, exp, log, erf, atan):
        self.exp, self.log, self.erf, self.atan = exp, log, erf, atan

    def exp1(self, v): return float(self.exp(np.array([v], dtype=np.float64))[0])
    def log1(self, v): return float(self.log(np.array([v], dtype=np.float64))[0])
    def erf1(self, v): return float(self.erf(np.array([v], dtype=np.float64))[0])
    def atan1(self, v): return float(self.atan(np.array([v], dtype=np.float64))[0])


def deterministic(oracle, smcmc):
    return Backend(oracle.det_exp, oracle.det_log,
                   lambda x: smcmc.selftest_detmath(10, x, device=-1), lambda x: smcmc.selftest_detmath(11, x, device=-1))


def libm():
    def lift(f):
        return lambda x: np.array([f(float(v)) for v in np.asarray(x, dtype=np.float64).ravel()], dtype=np.float64)
    return Backend(lift(math.exp), lift(math.log), lift(math.erf), lift(math.atan))


def split(params):
    """(nevents, nbins, xmin, xmax, exposure, cut, trueFakes, trueEfficiency, data[3 nbins], events[nevents][6])"""
    params = np.asarray(params, dtype=np.float64)
    nev, nbins = int(params[0]), int(params[1])
    data = params[8:8 + 3 * nbins]
    ev = params[8 + 3 * nbins:].reshape(nev, 6)
    return (nev, nbins) + tuple(float(v) for v in params[2:8]) + (data, ev)


def evaluate(params, point, be):
    """-> (logL, hist[3 nbins] as a list, where[nevents]: the flat bin an event was filled into, or a negative code:
    -1 mass > 500, -2 mass < 0, -3 separation < 0, -4 outside the axis)."""
    nev, nbins, xmin, xmax, exposure, cut, true_fakes, true_eff, data, ev = split(params)
    p = [float(v) for v in point]
    Mass, Type, Sep, MuDk, TrueMass, TrueSigma = (np.ascontiguousarray(ev[:, k]) for k in range(6))

    # SystematicCorrection.H:50-79, InvariantMass
    nominalLogMass = be.log(TrueMass)                          # :57
    nominalLogSigma = be.log(TrueMass + TrueSigma)             # :58
    nominalLogSigma = nominalLogSigma - nominalLogMass         # :59
    logMass = be.log(Mass)                                     # :61
    logSigma = (logMass - nominalLogMass) / nominalLogSigma    # :62
    scale = p[2] / 10.0                                        # :64
    width = be.exp1(p[3] / 10.0)                               # :65
    skew = 0.3 * be.erf1(p[4] / 10.0)                          # :68
    skewv = be.exp(logSigma * skew)                            # :69
    logMass = nominalLogMass + (logMass - nominalLogMass) * skewv    # :72
    logMass = nominalLogMass + (logMass - nominalLogMass) * width    # :73
    logMass = logMass + scale                                  # :74
    mass = be.exp(logMass)                                     # :76

    # :35-48, Separation
    sep_scale = (be.exp1(p[5] / 10.0), be.exp1(p[6] / 10.0))   # :40-43
    sep = Sep * np.where(Type > 0, sep_scale[1], sep_scale[0])  # :47

    # :81-117, EventWeight
    ws = be.exp1(p[0] / 10.0)                                  # :87
    wb = be.exp1(p[1] / 10.0)                                  # :88
    cf = math.tan(math.pi * (true_fakes - 0.5))                # :94 (a constant of the sample, from libm)
    cf += p[7]                                                 # :95
    cf = be.atan1(cf) / math.pi + 0.5                          # :96
    ce = math.tan(math.pi * (true_eff - 0.5))                  # :106
    ce += p[8]                                                 # :107
    ce = be.atan1(ce) / math.pi + 0.5                          # :108
    weight = {(0, 1): (ws * (cf / true_fakes)) * exposure,                     # :99, 115
              (0, 0): (ws * ((1.0 - cf) / (1.0 - true_fakes))) * exposure,     # :100, 115
              (1, 1): (wb * (ce / true_eff)) * exposure,                       # :111, 115
              (1, 0): (wb * ((1.0 - ce) / (1.0 - true_eff))) * exposure}       # :112, 115

    # FakeLikelihood.H:188-216, FillHistograms
    hist = [0.0] * (3 * nbins)
    where = [0] * nev
    for i in range(nev):
        m, s = float(mass[i]), float(sep[i])
        w = weight[(1 if Type[i] > 0 else 0, 1 if MuDk[i] > 0 else 0)]
        if m > 500.0:                                          # :203
            where[i] = -1
            continue
        if m < 0.0:                                            # :204
            where[i] = -2
            continue
        if s < 0.0:                                            # :205
            where[i] = -3
            continue
        if MuDk[i] > 0:                                        # :206
            h = 2
        elif s < cut:                                          # :210
            h = 0
        else:
            h = 1
        # TH1::Fill: the bin rule of smcmc.h
        if not (m >= xmin) or not (m < xmax):
            where[i] = -4
            continue
        b = int((float(nbins) * (m - xmin)) / (xmax - xmin))
        if b > nbins - 1:
            b = nbins - 1
        hist[h * nbins + b] = hist[h * nbins + b] + w
        where[i] = h * nbins + b

    # :47-81, operator()
    logl = 0.0
    for k in range(3 * nbins):                                 # Close, Separated, DecayTag
        d = float(data[k])
        mc = hist[k]
        if mc < 0.001:
            mc = 0.001
        v = d - mc
        if d > 0.0:
            v += d * be.log1(mc / d)
        logl += v
    return logl, hist, where


# ---- deterministic samples ---------------------------------------------------------------------------------------
class _Stream:
    """uniforms in (0, 1) from oracle.philox, a counter per draw"""
    def __init__(self, oracle, key):
        self.oracle, self.key, self.n, self.buf = oracle, [int(key), 0x5eed], 0, []

    def uniform(self):
        if not self.buf:
            self.buf = self.oracle.philox([self.n, 0, 0, 0], self.key)
            self.n += 1
        return (self.buf.pop() + 0.5) * 2.0 ** -32

    def gaus(self, mean, sigma):
        return mean + sigma * math.sqrt(-2.0 * math.log(self.uniform())) * math.cos(2.0 * math.pi * self.uniform())


def make_sample(oracle, nsignal, nbackground, nbins, key, xmin=0.0, xmax=500.0):
    """The flat parameter array of a toy sample (exposure ratio 1): the distributions of example/Simulated.H:31-53,
    and in it, by construction, an event whose separation is exactly the cut (signal, untagged), a background event
    far above xmax, both types and both MuDk values.  data: small counts everywhere except two bins of zero; it is
    returned with the array so that a test can set its own."""
    r = _Stream(oracle, key)
    ev = []
    for i in range(nsignal):                                   # MakeSignalEvent
        true_mass = 135.0
        sigma = 0.3 * true_mass
        mass = r.gaus(true_mass, sigma)
        while mass <= 0:
            mass = r.gaus(true_mass, sigma)
        sepn = abs(-100.0 * math.log(r.uniform()))
        mudk = 1 if r.uniform() < 0.05 else 0
        ev.append([mass, 0, sepn, mudk, true_mass, sigma])
    for i in range(nbackground):                               # MakeBackgroundEvent
        true_mass = 1000.0 * r.uniform()
        sigma = 0.3 * true_mass
        mass = r.gaus(true_mass, sigma)
        while mass <= 0:
            mass = r.gaus(true_mass, sigma)
        sepn = abs(r.gaus(0.0, 50.0))
        mudk = 1 if r.uniform() < 0.5 else 0
        ev.append([mass, 1 + (i % 2), sepn, mudk, true_mass, sigma])
    ev = np.array(ev, dtype=np.float64)
    ev[0, 2], ev[0, 3] = 100.0, 0          # exactly the cut, untagged: Separated
    ev[1, 3] = 1                           # a tagged signal event
    ev[nsignal, 0], ev[nsignal, 4], ev[nsignal, 5] = 731.0, 700.0, 210.0   # far above xmax
    ev[nsignal + 1, 3], ev[nsignal + 2, 3] = 1, 0
    data = np.array([[1 + (7 * h + 3 * b) % 23 for b in range(nbins)] for h in range(3)], dtype=np.float64)
    data[0, 1 % nbins] = 0.0
    data[2, nbins - 1] = 0.0
    head = [ev.shape[0], nbins, xmin, xmax, 1.0, 100.0, 0.05, 0.5]
    return np.concatenate([np.array(head, dtype=np.float64), data.ravel(), ev.ravel()])


def truncate(params, nevents):
    """The first nevents events of a sample, nevents rewritten: the samples below make_sample's two signal and three
    background events."""
    params = np.asarray(params, dtype=np.float64)
    nbins = int(params[1])
    assert 1 <= nevents <= int(params[0])
    out = params[:8 + 3 * nbins + 6 * nevents].copy()
    out[0] = nevents
    return out


def points(oracle, n, key, spread=3.0):
    """n points of nine coordinates: the origin, then uniform in (-spread, spread), the last with a mass skew beyond the
    switch of smcmc_erf's two forms (p[4] / 10 > 7/8)."""
    r = _Stream(oracle, key)
    out = [np.zeros(9)]
    for k in range(1, n):
        out.append(np.array([spread * (2.0 * r.uniform() - 1.0) for _ in range(9)]))
    out[-1][4] = 12.0
    return out


# ---- the arguments smcmc_erf / smcmc_atan are tested on: both signs, every branch of the implementation with its
# switch-over points +- 1 ulp, zeros, subnormals, huge arguments (inf and NaN are checked by name) ----
def _around(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def erf_grid():
    rng = np.random.default_rng(11)
    g = [rng.uniform(-7.0, 7.0, 20000), rng.uniform(-1.0, 1.0, 20000), rng.uniform(0.8, 2.5, 10000),
         np.exp(rng.uniform(-745.0, 3.0, 10000)), -np.exp(rng.uniform(-745.0, 3.0, 10000))]
    edges = []
    for v in (0.875, 6.0, 1.0, 0.5, 2.0 ** -28):               # the switch-over points of smcmc_erf, and some of libm's
        edges += _around(v) + [-t for t in _around(v)]
    g.append(np.array(edges + [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 26.0, -26.0, 1e300,
                               -1e300]))
    return np.concatenate(g)


def atan_grid():
    rng = np.random.default_rng(12)
    mag = np.exp(rng.uniform(math.log(1e-12), math.log(1e22), 40000))
    g = [mag[:20000], -mag[20000:], rng.uniform(-3.0, 3.0, 20000)]
    edges = []
    for v in (2.0 ** -29, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66, 1.0):   # every branch of smcmc_atan
        edges += _around(v) + [-t for t in _around(v)]
    g.append(np.array(edges + [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e300, -1e300]))
    return np.concatenate(g)
