"""SMCMC_LIKE_EVENT_TEMPLATE on the device: the ensemble kernel (frozen and pooled) and the one-chain-per-wavefront kernel
of SMCMC_MODE_PER_CHAIN against the restatement of tests/event_template_ref.py evaluated at the engine's own points,
the configurations the likelihood refuses, and examples/FakeMCMC2_amd.C.

As for SMCMC_LIKE_EVENT_SAMPLE the oracle has no event sample, so chain parity comes from the engine's own record: every
likelihood it reports is the restatement's at the point it reports, bit for bit, and every accept decision is the
reference's test (TSimpleMCMC.H:432-463) recomputed from the two recorded likelihoods and the engine's own uniform."""
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_event_template_cases", os.path.join(HERE, "event_template_cases.py"))
tcases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tcases)
tref, ref = tcases.tref, tcases.ref

pytestmark = pytest.mark.gpu
ERR_UNSUPPORTED = 5
SEED = 20260131
NCHAINS = tcases.NCHAINS


class Restatement:
    """the deterministic restatement of one sample, remembered by point"""
    def __init__(self, oracle, smcmc, params):
        self.params, self.be, self.seen = params, ref.deterministic(oracle, smcmc), {}

    def __call__(self, point):
        key = np.asarray(point, dtype=np.float64).tobytes()
        if key not in self.seen:
            self.seen[key] = tref.evaluate(self.params, point, self.be)[0]
        return self.seen[key]


SAMPLES = {"197ev_50bins": (60, 137, 50, 101), "64ev_5bins": (30, 34, 5, 102)}   # as tests/test_event_template_cpu.py


@pytest.fixture(scope="module", params=list(SAMPLES), ids=list(SAMPLES))
def sample(request, oracle, gpu):
    nsig, nbkg, nbins, key = SAMPLES[request.param]
    params = tref.interleave(tref.make_sample(oracle, nsig, nbkg, nbins, key), 3)     # (the engine partitions it)
    return params, Restatement(oracle, gpu, params)


@pytest.mark.parametrize("mode", ["frozen", "pooled"])
def test_ensemble_likelihoods_are_the_restatement(gpu, oracle, sample, mode):
    params, restate = sample
    eng = gpu.Engine(9, nchains=NCHAINS, likelihood=gpu.LIKE_EVENT_TEMPLATE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_FROZEN if mode == "frozen" else gpu.MODE_POOLED)
    eng.KeepProposed()
    x0 = tcases.starts(oracle, NCHAINS, 77, params)
    assert eng.Start(x0)
    logl = eng.lane("logl")
    assert np.array_equal(eng.GetAccepted(), x0)
    for c in range(NCHAINS):
        assert logl[c] == restate(x0[:, c]), "start, chain %d" % c
    if mode == "frozen":
        eng.Step(48)
    else:
        for _ in range(3):                           # 48 steps, a sync every 16
            eng.Step(16)
            eng.sync()
    x, xp = eng.GetAccepted(), eng.GetProposed()
    logl, loglp = eng.lane("logl"), eng.lane("logl_proposed")
    for c in range(NCHAINS):
        assert logl[c] == restate(x[:, c]), "accepted, chain %d" % c
        assert tref.same(loglp[c], restate(xp[:, c])), "proposed, chain %d" % c
    assert int(eng.lane("naccept").sum()) > 0 and not np.array_equal(x, x0)
    hist, l0 = eng.EventTemplateHistograms(x[:, 0])
    assert l0 == logl[0] and hist.shape == (3, int(params[1]))
    eng.close()


def test_one_chain_adapting_alone(gpu, oracle, sample):
    params, restate = sample
    nchains, nsteps = 3, 64
    eng = gpu.Engine(9, nchains=nchains, likelihood=gpu.LIKE_EVENT_TEMPLATE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_PER_CHAIN)
    assert eng.get_param("PERCHAIN_WAVE") == 1.0
    x0 = tcases.starts(oracle, nchains, 78, params)
    assert eng.Start(x0)
    start_logl = eng.lane("logl")
    for c in range(nchains):
        assert start_logl[c] == restate(x0[:, c])
    eng.snapshot()
    accepts = rejects = 0
    first = None
    for c in range(nchains):
        rec = eng.StepRecorded(nsteps, chain=c)
        if c == 0:
            first = rec
        prev = start_logl[c]
        for s in range(nsteps):
            lp, la = rec["logl_proposed"][s], rec["logl"][s]
            assert tref.same(lp, restate(rec["proposed"][s])), "proposed, chain %d step %d" % (c, s)
            assert la == restate(rec["accepted"][s]), "accepted, chain %d step %d" % (c, s)
            # TSimpleMCMC.H:432-463 from the engine's own draw
            step = int(rec["total_steps"][s])
            assert step == s + 1
            u = oracle.step_draws(SEED, c, step, 9)[1]
            take = math.isfinite(lp) and not lp < -0.999999E+30
            if take:
                delta = lp - prev
                if delta < 0.0 and delta < float(oracle.det_log(np.array([u]))[0]):
                    take = False
            assert int(rec["last_accept"][s]) == int(take), "accept test, chain %d step %d" % (c, s)
            assert la == (lp if take else prev)
            accepts, rejects = accepts + int(take), rejects + int(not take)
            prev = la
        eng.rollback()
    assert accepts > 0 and rejects > 0
    again = eng.StepRecorded(nsteps, chain=0)         # snapshot / rollback / replay: the same rows
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    eng.close()


def test_refusals(gpu, oracle, sample):
    params, _ = sample

    def refused(make, status=ERR_UNSUPPORTED):
        with pytest.raises(gpu.SmcmcError) as e:
            make()
        assert e.value.status == status
        assert len(str(e.value).split(":", 1)[1].strip()) > 0          # a message

    like = gpu.LIKE_EVENT_TEMPLATE
    refused(lambda: gpu.HmcEngine(9, nchains=4, likelihood=like, likelihood_params=params))
    refused(lambda: gpu.VaatEngine(9, nchains=4, likelihood=like, likelihood_params=params))
    refused(lambda: gpu.Engine(8, nchains=4, likelihood=like))
    refused(lambda: gpu.Engine(10, nchains=4, likelihood=like))
    refused(lambda: gpu.Engine(9, nchains=4, likelihood=like, likelihood_params=params, exact=False))
    eng = gpu.Engine(9, nchains=4, likelihood=like, likelihood_params=params, mode=gpu.MODE_PER_CHAIN)
    refused(lambda: eng.set_param("PERCHAIN_WAVE", 0))
    refused(lambda: eng.set_param("EXACT_ARITHMETIC", 0))

    def set_params(prm):
        prm = np.ascontiguousarray(prm, dtype=np.float64)
        eng._check(eng._lib.smcmc_set_likelihood_params(eng._h, prm.ctypes.data_as(gpu._capi._dp), prm.size))

    with pytest.raises(gpu.SmcmcError) as e:                           # the parameter rules hold on the engine too
        set_params(params[:-1])
    assert e.value.status == 1 and "exactly" in str(e.value)
    bad = params.copy(); bad[4] = 0.5
    with pytest.raises(gpu.SmcmcError) as e:                           # ... the three of this likelihood among them
        set_params(bad)
    assert e.value.status == 1 and "exposureRatio" in str(e.value)
    bad = params.copy(); bad[8 + 3 * int(params[1]) + 1::6] = 0.0
    with pytest.raises(gpu.SmcmcError) as e:
        set_params(bad)
    assert e.value.status == 1 and "background" in str(e.value)
    assert eng.Start(tcases.starts(oracle, 4, 5, params))              # and the engine is still good
    eng.close()


def test_fake_mcmc2_example(gpu, tmp_path):
    """examples/FakeMCMC2_amd.C (example2/FakeMCMC.C on the mirror) with a small Init(40, 40, 2.0): two burn-ins of 50 and
    100 steps, four legs of 100 saved steps; the last entry's LogLikelihood is the host definition at that entry's
    Accepted."""
    root = os.path.dirname(HERE)
    libdir = os.path.join(root, "root-simple-mcmc_amd", "lib")
    exe = str(tmp_path / "fake_mcmc2_amd.exe")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(root, 'include')}",
           os.path.join(root, "examples", "FakeMCMC2_amd.C"), f"-L{libdir}", "-lsmcmc_amd",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, prm_path = tmp_path / "fake2.csv", tmp_path / "params.txt"
    r = subprocess.run([exe, "40", "40", "2.0", "100", "100", str(out), str(prm_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Start new burnin phase (50 steps)" in r.stdout and "Start new burnin phase (100 steps)" in r.stdout
    assert "12 histograms kept" in r.stdout                              # initial, burnin1, burnin2, midway (rewritten)
    lines = open(out).read().splitlines()
    col = {h: i for i, h in enumerate(lines[0].split(",")) if h}
    rows = [l.split(",") for l in lines[1:]]
    assert len(rows) == 400
    params = np.loadtxt(prm_path)
    assert int(params[1]) == 50 and params[4] == 1.0 and int(params[0]) > 2000    # the floors of example2/Simulated.H
    last = rows[-1]
    x = np.array([float(last[col[f"Accepted[{d}]"]]) for d in range(9)])
    assert float(last[col["LogLikelihood"]]) == gpu.event_template_evaluate(params, x)
    logl = np.array([float(r_[col["LogLikelihood"]]) for r_ in rows])
    assert np.all(np.isfinite(logl)) and len(np.unique(logl)) > 10       # the chain moves
