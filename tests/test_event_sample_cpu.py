"""SMCMC_LIKE_EVENT_SAMPLE without a GPU: the deterministic erf / atan on the host against libm, the host definition
(smcmc_event_sample_evaluate) against the restatement of tests/event_sample_ref.py bit for bit, the deterministic
restatement against the libm one, and the rules of the parameter array."""
import importlib.util
import math
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("smcmc_event_sample_ref",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_sample_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

ERR_INVALID = 1


def _ulps(a, b):
    """|a - b| in units of the spacing of b (b: libm's value)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.spacing(np.abs(b))
    d[(a == b)] = 0.0          # equal infinities
    return d


def test_erf_host_within_two_ulp_of_libm(smcmc):
    x = ref.erf_grid()
    got = smcmc.selftest_detmath(10, x, device=-1)
    want = np.array([math.erf(v) for v in x])
    err = _ulps(got, want)
    print("smcmc_erf: largest difference from libm %.2f ulp at x = %r" % (err.max(), float(x[np.argmax(err)])))
    assert err.max() <= 2.0
    assert np.array_equal(np.signbit(got), np.signbit(x))                       # odd, -0 included
    sp = smcmc.selftest_detmath(10, np.array([np.inf, -np.inf, np.nan]), device=-1)
    assert sp[0] == 1.0 and sp[1] == -1.0 and np.isnan(sp[2])


def test_atan_host_within_two_ulp_of_libm(smcmc):
    x = ref.atan_grid()
    got = smcmc.selftest_detmath(11, x, device=-1)
    want = np.array([math.atan(v) for v in x])
    err = _ulps(got, want)
    print("smcmc_atan: largest difference from libm %.2f ulp at x = %r" % (err.max(), float(x[np.argmax(err)])))
    assert err.max() <= 2.0
    assert np.array_equal(np.signbit(got), np.signbit(x))
    sp = smcmc.selftest_detmath(11, np.array([np.inf, -np.inf, np.nan]), device=-1)
    assert sp[0] == math.pi / 2 and sp[1] == -math.pi / 2 and np.isnan(sp[2])


def test_host_kinds_are_the_oracles_functions(smcmc, oracle):
    """device = -1 evaluates include/smcmc_detmath.h on the host: for log and exp that is what the oracle compiles"""
    rng = np.random.default_rng(13)
    x = np.exp(rng.uniform(-50, 50, 1000))
    assert np.array_equal(smcmc.selftest_detmath(0, x, device=-1), oracle.det_log(x))
    t = rng.uniform(-50, 50, 1000)
    assert np.array_equal(smcmc.selftest_detmath(1, t, device=-1), oracle.det_exp(t))
    with pytest.raises(smcmc.SmcmcError) as e:
        smcmc.selftest_detmath(5, x, device=-1)
    assert e.value.status == ERR_INVALID


CASES = [(60, 137, 50, 101), (30, 34, 5, 102)]    # signal, background (197 and 64 events), nbins, key


@pytest.fixture(scope="module", params=CASES, ids=["197ev_50bins", "64ev_5bins"])
def case(request, oracle, smcmc):
    nsig, nbkg, nbins, key = request.param
    params = ref.make_sample(oracle, nsig, nbkg, nbins, key)
    pts = ref.points(oracle, 12, key + 1000)
    det = [ref.evaluate(params, p, ref.deterministic(oracle, smcmc)) for p in pts]
    return params, pts, det, nsig, nbins


def test_fixture_has_the_cases_the_definition_branches_on(case):
    params, pts, det, nsig, nbins = case
    nev, nb, xmin, xmax, exposure, cut, tf, te, data, ev = ref.split(params)
    assert nev == nsig + (137 if nbins == 50 else 34) and nb == nbins
    assert set(ev[:, 1] > 0) == {True, False} and set(ev[:, 3] > 0) == {True, False}
    for signal in (True, False):
        for tagged in (True, False):
            assert np.any(((ev[:, 1] > 0) != signal) & ((ev[:, 3] > 0) == tagged))
    logl0, hist0, where0 = det[0]                       # the origin
    assert ev[0, 2] == cut and nbins <= where0[0] < 2 * nbins          # exactly the cut: Separated
    for (logl, hist, where), p in zip(det, pts):
        assert where[nsig] == -1                                       # corrected mass above xmax
        assert any(m < 0.001 and d > 0 for m, d in zip(hist, data))    # the 0.001 clamp opposite data
        assert any(d == 0 for d in data)                               # the data > 0 branch not taken
        assert math.isfinite(logl)
    assert data.sum() <= 1e4


def test_host_definition_is_the_restatement_bit_for_bit(case, smcmc):
    params, pts, det, nsig, nbins = case
    for p, (logl, hist, where) in zip(pts, det):
        got, h = smcmc.event_sample_evaluate(params, p, histograms=True)
        assert np.array_equal(h.ravel(), np.array(hist))
        assert got == logl


def test_deterministic_restatement_against_libm(case):
    params, pts, det, nsig, nbins = case
    be = ref.libm()
    worst = 0.0
    for p, (logl, hist, where) in zip(pts, det):
        l2, h2, w2 = ref.evaluate(params, p, be)
        assert w2 == where             # no event changes bin or cut between the two backends
        worst = max(worst, abs(l2 - logl))
    print("event sample, %d bins: largest |logL(deterministic) - logL(libm)| = %.3e" % (nbins, worst))
    assert worst <= 1e-9


def test_exposure_ratio_as_init_takes_it(case, smcmc):
    """event_sample_params with no ratio given: FakeLikelihood::Init's data / mc (FakeLikelihood.H:107-138)"""
    params, pts, det, nsig, nbins = case
    nev, nb, xmin, xmax, exposure, cut, tf, te, data, ev = ref.split(params)
    prm = smcmc.event_sample_params(ev, data.reshape(3, nbins), nbins, xmin, xmax)
    logl, hist, where = det[0]
    d = m = 0.0
    for h in range(3):
        sd = sm = 0.0
        for b in range(nbins):
            sd += float(data[h * nbins + b])
            sm += hist[h * nbins + b]
        d, m = (sd, sm) if h == 0 else (d + sd, m + sm)
    assert prm[4] == d / m and prm.size == params.size
    assert np.array_equal(np.delete(prm, 4), np.delete(params, 4))


def test_parameter_rules(case, smcmc, oracle):
    params, pts, det, nsig, nbins = case
    nev = int(params[0])
    ev0 = 8 + 3 * nbins

    def refused(prm, text):
        with pytest.raises(smcmc.SmcmcError) as e:
            smcmc.event_sample_evaluate(prm, np.zeros(9))
        assert e.value.status == ERR_INVALID and text in str(e.value)

    smcmc.event_sample_evaluate(params, np.zeros(9))                   # the array itself is fine
    refused(params[:-1], "exactly")                                    # a wrong count
    refused(np.append(params, 0.0), "exactly")
    refused(params[:5], "EVENT_SAMPLE needs")
    for bad_bins in (0.0, smcmc._capi.EVENT_SAMPLE_MAX_BINS + 1.0, 2.5):
        prm = params.copy(); prm[1] = bad_bins
        refused(prm, "nbins")
    prm = params.copy(); prm[0] = 0.0
    refused(prm, "nevents")
    for k, v in ((4, np.inf), (2, np.nan), (8 + 3, np.inf), (ev0 + 2, np.nan), (ev0 + 6 * (nev - 1) + 5, -np.inf)):
        prm = params.copy(); prm[k] = v
        refused(prm, "not finite")
    for field in (0, 4, 5):                                            # Mass, TrueMass, TrueMassSigma
        for v in (0.0, -1.0):
            prm = params.copy(); prm[ev0 + 6 * 3 + field] = v
            refused(prm, "must be > 0")
    prm = params.copy(); prm[ev0 + 1] = -1.0                           # a data event in the simulated sample
    refused(prm, "Type")
    # the largest nbins is served
    big = ref.make_sample(oracle, 5, 5, smcmc._capi.EVENT_SAMPLE_MAX_BINS, 7)
    assert math.isfinite(smcmc.event_sample_evaluate(big, np.zeros(9)))



def test_fake_mcmc_example_compiles(smcmc, tmp_path):
    """examples/FakeMCMC_amd.C and include/FakeLikelihood_amd.H build against the library, warnings as errors"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "root-simple-mcmc_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(root, 'include')}",
           os.path.join(root, "examples", "FakeMCMC_amd.C"), f"-L{libdir}", "-lsmcmc_amd",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "fake_mcmc_amd.exe")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
