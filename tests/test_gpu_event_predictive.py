"""smcmc_event_predictive_sums on the device: the histograms of the three likelihoods over a simulated event sample at every
point of a saved trace, and their sums per bin.

  1  every point's histograms and log-likelihood are the host evaluator's, bit for bit and NaN as NaN, on hand-made
     traces whose padding lanes and rows >= dim are NaN: the samples of the ensemble kernels' own tests (largest LDS, one
     bin, event counts around the batch of four, the class boundary around a batch) on traces of one lane, 63 of 64, 65 of
     128 and 130 of 256 lanes (a whole dead block)
  2  the sums against math.fsum of the very terms the device adds, within the bound any order of additions keeps; the
     same bits from a second call, without the optional outputs, and with other contents in the padding
  3  an engine's own saved trace: the log-likelihood recomputed here is the one the step kernel saved, bit for bit
  4  the refusals of tests/test_event_predictive_cpu.py write nothing with a device present
"""
import ctypes as C
import importlib.util
import math
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

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)
SEED = 20260131
# nslots, nchains, nchains_padded: one lane; one short of a wavefront; a second block of one lane; a whole dead block
SAMPLE_SHAPES = [(1, 1, 64), (2, 63, 64), (5, 65, 128), (3, 130, 256)]
TEMPLATE_SHAPES = [(2, 65, 128), (3, 130, 256)]
SHAPE_SHAPES = [(2, 65, 128)]
U = 2.0 ** -53


def same(a, b):
    """bit for bit (a zero's sign included), NaN compared as NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))))


class Member:
    """one likelihood of the family over one sample: its pool of points and the host evaluator's values at them, taken once"""

    def __init__(self, gpu, oracle, member, params, key):
        self.member, self.params = member, np.ascontiguousarray(params, dtype=np.float64)
        nbins = int(params[1])
        if member == "sample":
            self.like, self.dim, self.nh, self.strides = gpu.LIKE_EVENT_SAMPLE, 9, 3, (15, 9)
            pool = list(ref.points(oracle, cases.NPOINTS, key)) + list(cases.extreme_points())
            evaluate = gpu.event_sample_evaluate
        elif member == "template":
            self.like, self.dim, self.nh, self.strides = gpu.LIKE_EVENT_TEMPLATE, 9, 3, (15, 9)
            pool = list(tref.points(oracle, cases.NPOINTS, key, params))
            total = float(np.sum(params[8:8 + 3 * nbins]))
            for p in cases.extreme_points():
                p[0], p[1] = 0.4 * total, 0.6 * total
                pool.append(p)
            evaluate = gpu.event_template_evaluate
        else:
            self.like, self.dim, self.nh, self.strides = gpu.LIKE_EVENT_SHAPE, 31, 4, (31, 33)
            pool = list(sref.points(oracle, cases.NPOINTS, key, params)) + list(sref.extreme_points(params))
            evaluate = gpu.event_shape_evaluate
        self.rows = self.nh * nbins
        self.pool = np.array(pool)                                          # [npool][dim]
        values = [evaluate(self.params, p, histograms=True) for p in self.pool]
        self.logl = np.array([v[0] for v in values])
        self.hist = np.array([v[1].ravel() for v in values])                # [npool][rows]
        self.finite = np.flatnonzero(np.all(np.isfinite(self.hist), axis=1))

    def deal(self, nslots, nchains, only=None):
        """which point of the pool (or of its subset `only`) sits at (slot, chain): neighbouring lanes and neighbouring
        slots hold different points"""
        ids = np.arange(len(self.pool)) if only is None else np.asarray(only)
        assert len(ids) > 5
        t, c = np.meshgrid(np.arange(nslots), np.arange(nchains), indexing="ij")
        return ids[(c + 5 * t) % len(ids)]

    def trace(self, idx, npad, dim_stride, padding=float("nan")):
        """the device trace [slot][dim_stride][npad] of the dealt points; padding lanes and rows >= dim hold `padding`"""
        import torch
        nslots, nchains = idx.shape
        x = np.transpose(self.pool[idx], (0, 2, 1))                         # [slot][dim][chain]
        trace = torch.full((nslots, dim_stride, npad), padding, dtype=torch.float64, device="cuda")
        trace[:, :self.dim, :nchains] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
        torch.cuda.synchronize()
        return trace

    def run(self, gpu, trace, nslots, dim_stride, nchains, npad, centre=None, outputs=True):
        """(status, sum, sumsq, hist[slot][rows][npad] or None, logl[slot][npad] or None); every output prefilled"""
        import torch
        s, q = np.full(self.rows, -7.0), np.full(self.rows, -7.0)
        h = torch.full((nslots, self.rows, npad), -7.0, dtype=torch.float64, device="cuda") if outputs else None
        l = torch.full((nslots, npad), -7.0, dtype=torch.float64, device="cuda") if outputs else None
        torch.cuda.synchronize()
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
        st = gpu.load().smcmc_event_predictive_sums(
            self.like, self.params.ctypes.data_as(DP), self.params.size, C.c_void_p(trace.data_ptr()), nslots, dim_stride, nchains,
            npad, None if c is None else c.ctypes.data_as(DP), C.c_void_p(h.data_ptr()) if outputs else None,
            C.c_void_p(l.data_ptr()) if outputs else None, s.ctypes.data_as(DP), q.ctypes.data_as(DP), None)
        torch.cuda.synchronize()
        return st, s, q, (h.cpu().numpy() if outputs else None), (l.cpu().numpy() if outputs else None)

    def check_points(self, gpu, what, shapes):
        """test 1 on every trace shape and both strides"""
        for nslots, nchains, npad in shapes:
            idx = self.deal(nslots, nchains)
            for stride in self.strides:
                where = "%s: %d slots, %d / %d lanes, stride %d" % (what, nslots, nchains, npad, stride)
                st, s, q, h, l = self.run(gpu, self.trace(idx, npad, stride), nslots, stride, nchains, npad)
                assert st == 0, where
                want_h = np.transpose(self.hist[idx], (0, 2, 1))            # [slot][rows][chain]
                assert same(h[:, :, :nchains], want_h), where
                assert same(l[:, :nchains], self.logl[idx]), where
                assert same(h[:, :, nchains:], np.zeros((nslots, self.rows, npad - nchains))), where     # +0.0
                assert same(l[:, nchains:], np.zeros((nslots, npad - nchains))), where


SAMPLE_NAMES = ["65ev_97bins", "45ev_1bin", "1ev_5bins", "3ev_5bins", "5ev_5bins", "197ev_50bins"]


@pytest.mark.parametrize("name", SAMPLE_NAMES)
def test_event_sample_points_are_the_hosts(gpu, oracle, name):
    """97 bins: the largest dynamic LDS of the kernel; 1 bin: three rows and the spare one; 1, 3, 5 events: around the
    batch of four"""
    m = Member(gpu, oracle, "sample", cases.sample(ref, oracle, name), cases.CASES[name][3] + 1000)
    assert np.isfinite(m.hist).all() and not m.hist[-2].any() and m.hist[-1].any()      # the extreme points: all dropped; the first bins
    m.check_points(gpu, name, SAMPLE_SHAPES)


def _template_samples(oracle):
    out = {n: tcases.binned(oracle, spec) for n, spec in tcases.ENSEMBLE_BINS.items()}
    for counts in ((1, 1), (5, 1), (1, 5)):
        out["%dsig_%dbkg" % counts] = tcases.counted(oracle, "ensemble", *counts)
    out["interleaved"] = tref.interleave(tref.make_sample(oracle, 30, 34, 5, 102), 5)
    return out


TEMPLATE_NAMES = ["97bins", "1bin", "1sig_1bkg", "5sig_1bkg", "1sig_5bkg", "interleaved"]


@pytest.mark.parametrize("name", TEMPLATE_NAMES)
def test_event_template_points_are_the_hosts(gpu, oracle, name):
    """97 bins: the most rows of a park column; the class boundary around a batch of four; events the caller did not sort
    by class"""
    m = Member(gpu, oracle, "template", _template_samples(oracle)[name], 1300 + TEMPLATE_NAMES.index(name))
    assert np.isnan(m.hist[-2]).all() and len(m.finite) >= 6            # every event dropped: both integrals 0
    m.check_points(gpu, name, TEMPLATE_SHAPES)


def _shape_samples(oracle):
    out = {n: scases.binned(oracle, spec) for n, spec in scases.ENSEMBLE_BINS.items()}
    for counts in ((1, 1), (4, 4)):
        out["%dsig_%dbkg" % counts] = scases.counted(oracle, "ensemble", *counts)
    return out


SHAPE_NAMES = ["maxbins", "1bin", "1sig_1bkg", "4sig_4bkg"]


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_event_shape_points_are_the_hosts(gpu, oracle, name):
    """SMCMC_EVENT_SHAPE_MAX_BINS: the largest dynamic LDS (histograms, spare row, tables)"""
    assert scases.MAX_BINS == 59
    m = Member(gpu, oracle, "shape", _shape_samples(oracle)[name], 1400 + SHAPE_NAMES.index(name))
    assert np.isnan(m.hist[-2]).all() and len(m.finite) >= 6
    m.check_points(gpu, name, SHAPE_SHAPES)


def _gamma(k):
    return k * U / (1.0 - k * U)


def _check_sums(m, s, q, h, centre, nchains, what):
    """sum and sumsq against math.fsum of the device's own terms y = h - centre and y * y (both exact in numpy: one IEEE
    operation each), h the histograms test 1 pinned.  Any order of adding n doubles errs by at most gamma_(n-1) sum|term|
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); asserted: gamma_(n+1).  A row with a NaN term
    is NaN."""
    y = h[:, :, :nchains] - (0.0 if centre is None else centre[None, :, None])
    yy = y * y
    n = y.shape[0] * nchains
    for name, got, terms in (("sum", s, y), ("sumsq", q, yy)):
        for r in range(m.rows):
            t = terms[:, r, :].ravel()
            if np.isnan(t).any():
                assert np.isnan(got[r]), "%s: %s[%d] should be NaN" % (what, name, r)
                continue
            exact, bound = math.fsum(t), _gamma(n + 1) * math.fsum(np.abs(t))
            print("%s %s[%d]: device %r exact %r bound %.3e" % (what, name, r, got[r], exact, bound))
            assert abs(got[r] - exact) <= bound, "%s: %s[%d] = %r, exact %r, bound %r" % (what, name, r, got[r], exact, bound)


SUM_CASES = {"sample": (5, 65, 128), "template": (2, 65, 128), "shape": (2, 65, 128)}


def _sum_member(gpu, oracle, member):
    if member == "sample":
        return Member(gpu, oracle, member, cases.sample(ref, oracle, "197ev_50bins"), 1101)
    if member == "template":
        return Member(gpu, oracle, member, tcases.counted(oracle, "ensemble", 5, 1), 1303)
    return Member(gpu, oracle, member, scases.counted(oracle, "ensemble", 4, 4), 1403)


@pytest.mark.parametrize("member", list(SUM_CASES))
def test_sums_are_the_sums_of_the_histograms(gpu, oracle, member):
    m = _sum_member(gpu, oracle, member)
    nslots, nchains, npad = SUM_CASES[member]
    stride = m.strides[0]                                                    # the engine's own: dim_padded
    eng = gpu.Engine(m.dim, nchains=nchains, likelihood=m.like, likelihood_params=m.params, seed=SEED, mode=gpu.MODE_FROZEN)
    assert eng.dim_padded == stride and eng.nchains_padded == npad
    near = 1.01 * np.mean(m.hist[m.finite], axis=0)                          # a centre near the mean
    # the trace of test 1 (for the two-pass members it holds the point whose histograms are NaN), then one of the finite
    # points alone, so that every member's rows meet the bound
    for only in (None, m.finite):
        idx = m.deal(nslots, nchains, only)
        trace = m.trace(idx, npad, stride)
        for centre in (None, near):
            what = "%s, %s, %s" % (member, "every point" if only is None else "finite points", "origin" if centre is None else "centre")
            st, s, q, h, l = m.run(gpu, trace, nslots, stride, nchains, npad, centre)
            assert st == 0 and same(h[:, :, :nchains], np.transpose(m.hist[idx], (0, 2, 1))), what
            _check_sums(m, s, q, h, centre, nchains, what)
            if only is not None:
                assert np.isfinite(s).all() and np.isfinite(q).all(), what
            st2, s2, q2, _, _ = m.run(gpu, trace, nslots, stride, nchains, npad, centre)
            assert st2 == 0 and same(s2, s) and same(q2, q), what + ": a second call"
            st3, s3, q3, _, _ = m.run(gpu, trace, nslots, stride, nchains, npad, centre, outputs=False)
            assert st3 == 0 and same(s3, s) and same(q3, q), what + ": without the optional outputs"
            other = m.trace(idx, npad, stride, padding=-3.0e5)               # finite points of large magnitude in the padding
            st4, s4, q4, h4, l4 = m.run(gpu, other, nslots, stride, nchains, npad, centre)
            assert st4 == 0 and same(s4, s) and same(q4, q) and same(h4, h) and same(l4, l), what + ": other padding"
            pp = eng.PosteriorPredictive(trace.data_ptr(), nslots, centre=None if centre is None else centre.reshape(m.nh, -1))
            n = float(nslots * nchains)
            assert pp.n == n and same(pp.sum.ravel(), s) and same(pp.sumsq.ravel(), q), what
            assert same(pp.mean.ravel(), (0.0 if centre is None else centre) + s / n), what
            assert pp.data.shape == (m.nh, m.rows // m.nh) and len(pp.names) == m.nh
    eng.close()
    gauss = gpu.Engine(9, nchains=64)
    with pytest.raises(gpu.SmcmcError) as err:
        gauss.PosteriorPredictive(trace.data_ptr(), 1)
    assert err.value.status == 2                                             # SMCMC_ERR_LOGIC: not the family's likelihood
    gauss.close()


def _end_to_end(gpu, m, x0, mode):
    import torch
    nchains, nslots = 130, 8
    eng = gpu.Engine(m.dim, nchains=nchains, likelihood=m.like, likelihood_params=m.params, seed=SEED, mode=mode)
    npad, stride = eng.nchains_padded, eng.dim_padded
    assert eng.Start(x0)
    x = torch.full((nslots, stride, npad), float("nan"), dtype=torch.float64, device="cuda")
    logl = torch.full((nslots, npad), float("nan"), dtype=torch.float64, device="cuda")
    again = torch.full((nslots, npad), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if mode == gpu.MODE_POOLED:
        eng.sync()
    eng.StepSave(32, x.data_ptr(), logl.data_ptr(), stride=4)
    if mode == gpu.MODE_POOLED:
        eng.sync()
    torch.cuda.synchronize()
    pp = eng.PosteriorPredictive(x.data_ptr(), nslots, logl_ptr=again.data_ptr())
    torch.cuda.synchronize()
    saved, got = logl.cpu().numpy()[:, :nchains], again.cpu().numpy()[:, :nchains]
    assert np.isfinite(saved).all()
    assert same(got, saved)
    assert same(again.cpu().numpy()[:, nchains:], np.zeros((nslots, npad - nchains)))
    xs = x.cpu().numpy()[:, :m.dim, :nchains]
    assert not np.array_equal(xs[0], xs[-1])                                 # the chains moved
    assert pp.n == 8 * 130 and pp.mean.shape == pp.spread.shape == (m.nh, m.rows // m.nh)
    ok = np.isfinite(pp.mean)
    assert ok.any() and np.all(np.isfinite(pp.spread[ok])) and np.all(pp.spread[ok] >= 0.0)
    # the same product about its own mean: the spread's difference cancels less
    near = eng.PosteriorPredictive(x.data_ptr(), nslots, centre=np.where(ok, pp.mean, 0.0))
    np.testing.assert_allclose(near.mean[ok], pp.mean[ok], rtol=1e-12, atol=0)
    eng.close()


@pytest.mark.parametrize("mode", ["frozen", "pooled"])
def test_end_to_end_event_sample(gpu, oracle, mode):
    """130 chains, 32 steps saved every fourth: the step kernel's saved log-likelihood of 1 040 points is the one this
    kernel finds at the saved points"""
    m = Member(gpu, oracle, "sample", cases.sample(ref, oracle, "197ev_50bins"), 1101)
    r = ref._Stream(oracle, 77)
    x0 = np.array([[2.0 * r.uniform() - 1.0 for _ in range(130)] for _ in range(9)])
    _end_to_end(gpu, m, x0, gpu.MODE_FROZEN if mode == "frozen" else gpu.MODE_POOLED)


def test_end_to_end_event_template(gpu, oracle):
    m = Member(gpu, oracle, "template", tcases.binned(oracle, tcases.ENSEMBLE_BINS["97bins"]), 1300)
    _end_to_end(gpu, m, tcases.starts(oracle, 130, 77, m.params), gpu.MODE_FROZEN)


def test_end_to_end_event_shape(gpu, oracle):
    m = Member(gpu, oracle, "shape", scases.binned(oracle, scases.ENSEMBLE_BINS["maxbins"]), 1400)
    _end_to_end(gpu, m, scases.starts(oracle, 130, 77, m.params), gpu.MODE_FROZEN)


def test_refusals_write_nothing_with_a_device(gpu, oracle):
    """the INVALID cases of tests/test_event_predictive_cpu.py on a real trace: the status, and every output untouched"""
    import torch
    m = Member(gpu, oracle, "sample", cases.sample(ref, oracle, "5ev_5bins"), 1102)
    t = Member(gpu, oracle, "template", tcases.counted(oracle, "ensemble", 4, 4), 1304)
    sh = Member(gpu, oracle, "shape", scases.counted(oracle, "ensemble", 4, 4), 1404)
    lib = gpu.load()

    def call(mem, like=None, params=None, count=None, nslots=2, stride=None, nchains=3, npad=64, give_sum=True, give_trace=True):
        params = mem.params if params is None else params
        stride = mem.strides[0] if stride is None else stride
        trace = torch.zeros((2, max(stride, mem.dim), 128), dtype=torch.float64, device="cuda")
        h = torch.full((2, mem.rows, 128), -7.0, dtype=torch.float64, device="cuda")
        l = torch.full((2, 128), -7.0, dtype=torch.float64, device="cuda")
        s, q = np.full(mem.rows, -7.0), np.full(mem.rows, -7.0)
        torch.cuda.synchronize()
        st = lib.smcmc_event_predictive_sums(mem.like if like is None else like, params.ctypes.data_as(DP),
                                             params.size if count is None else count,
                                             C.c_void_p(trace.data_ptr()) if give_trace else None, nslots, stride, nchains, npad,
                                             None, C.c_void_p(h.data_ptr()), C.c_void_p(l.data_ptr()),
                                             s.ctypes.data_as(DP) if give_sum else None, q.ctypes.data_as(DP), None)
        torch.cuda.synchronize()
        untouched = bool((h == -7.0).all()) and bool((l == -7.0).all()) and np.all(s == -7.0) and np.all(q == -7.0)
        return st, untouched

    def text():
        return lib.smcmc_event_sample_last_error().decode()

    assert call(m, like=0) == (1, True)
    assert call(m, like=10) == (1, True)
    assert call(m, count=m.params.size - 1) == (1, True) and "exactly" in text()
    half = t.params.copy()
    half[4] = 0.5
    assert call(t, params=half) == (1, True) and "exposureRatio" in text()
    assert call(m, stride=8) == (1, True)
    assert call(sh, stride=30) == (1, True)
    assert call(m, npad=65) == (1, True)
    assert call(m, nslots=0) == (1, True)
    assert call(m, give_sum=False) == (1, True)
    assert call(m, give_trace=False) == (1, True)
    assert call(m) == (0, False) and text() == ""                           # and the well-formed call runs
