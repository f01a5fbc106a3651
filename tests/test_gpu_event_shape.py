"""SMCMC_LIKE_EVENT_SHAPE on the device: the ensemble kernel (frozen and pooled) and the one-chain-per-wavefront kernel of
SMCMC_MODE_PER_CHAIN against the restatement of tests/event_shape_ref.py evaluated at the engine's own points, the
configurations the likelihood refuses, and examples/FakeMCMC3_amd.C.

As for the other event likelihoods the oracle has no event sample, so chain parity comes from the engine's own record:
every likelihood it reports is the restatement's at the point it reports, bit for bit, and every accept decision is the
reference's test (TSimpleMCMC.H:432-463) recomputed from the two recorded likelihoods and the engine's own uniform."""
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_event_shape_cases", os.path.join(HERE, "event_shape_cases.py"))
scases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(scases)
sref, ref = scases.sref, scases.ref

pytestmark = pytest.mark.gpu
ERR_UNSUPPORTED = 5
SEED = 20260131
NCHAINS = scases.NCHAINS
DIM = 31


class Restatement:
    """the deterministic restatement of one sample, remembered by point"""
    def __init__(self, oracle, smcmc, params):
        self.params, self.be, self.seen = params, ref.deterministic(oracle, smcmc), {}
        _, parts = smcmc.event_shape_evaluate(params, np.zeros(DIM), parts=True)
        self.kinv = (parts["KinvB"], parts["KinvS"])

    def __call__(self, point):
        key = np.asarray(point, dtype=np.float64).tobytes()
        if key not in self.seen:
            self.seen[key] = sref.evaluate(self.params, point, self.be, *self.kinv)[0]
        return self.seen[key]


SAMPLES = {"197ev_50bins": (60, 137, 50, 201), "64ev_5bins": (30, 34, 5, 202)}   # as tests/test_event_shape_cpu.py


@pytest.fixture(scope="module", params=list(SAMPLES), ids=list(SAMPLES))
def sample(request, oracle, gpu):
    nsig, nbkg, nbins, key = SAMPLES[request.param]
    params = sref.interleave(sref.make_sample(oracle, nsig, nbkg, nbins, key), 3)     # (the engine partitions it)
    return params, Restatement(oracle, gpu, params)


@pytest.mark.parametrize("mode", ["frozen", "pooled"])
def test_ensemble_likelihoods_are_the_restatement(gpu, oracle, sample, mode):
    params, restate = sample
    eng = gpu.Engine(DIM, nchains=NCHAINS, likelihood=gpu.LIKE_EVENT_SHAPE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_FROZEN if mode == "frozen" else gpu.MODE_POOLED)
    eng.KeepProposed()
    x0 = scases.starts(oracle, NCHAINS, 77, params)
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
        assert sref.same(loglp[c], restate(xp[:, c])), "proposed, chain %d" % c
    assert int(eng.lane("naccept").sum()) > 0 and not np.array_equal(x, x0)
    eng.close()


def test_event_shape_histograms(gpu, oracle, sample):
    params, restate = sample
    eng = gpu.Engine(DIM, nchains=4, likelihood=gpu.LIKE_EVENT_SHAPE, likelihood_params=params, seed=SEED)
    x0 = scases.starts(oracle, 4, 79, params)
    assert eng.Start(x0)
    hist, l0 = eng.EventShapeHistograms(x0[:, 0])
    want = sref.evaluate(params, x0[:, 0], restate.be, *restate.kinv)
    assert l0 == eng.lane("logl")[0] == want[0]
    assert hist.shape == (4, int(params[1])) and sref.same(hist.ravel(), want[1])
    eng.close()
    plain = gpu.Engine(5, nchains=4)
    with pytest.raises(gpu.SmcmcError):
        plain.EventShapeHistograms(np.zeros(DIM))
    plain.close()


def test_one_chain_adapting_alone(gpu, oracle, sample):
    params, restate = sample
    nchains, nsteps = 3, 64
    eng = gpu.Engine(DIM, nchains=nchains, likelihood=gpu.LIKE_EVENT_SHAPE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_PER_CHAIN)
    assert eng.get_param("PERCHAIN_WAVE") == 1.0
    x0 = scases.starts(oracle, nchains, 78, params)
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
            assert sref.same(lp, restate(rec["proposed"][s])), "proposed, chain %d step %d" % (c, s)
            assert la == restate(rec["accepted"][s]), "accepted, chain %d step %d" % (c, s)
            # TSimpleMCMC.H:432-463 from the engine's own draw
            step = int(rec["total_steps"][s])
            assert step == s + 1
            u = oracle.step_draws(SEED, c, step, DIM)[1]
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

    like = gpu.LIKE_EVENT_SHAPE
    refused(lambda: gpu.HmcEngine(DIM, nchains=4, likelihood=like, likelihood_params=params))
    refused(lambda: gpu.VaatEngine(DIM, nchains=4, likelihood=like, likelihood_params=params))
    refused(lambda: gpu.Engine(30, nchains=4, likelihood=like))
    refused(lambda: gpu.Engine(32, nchains=4, likelihood=like))
    refused(lambda: gpu.Engine(9, nchains=4, likelihood=like))
    refused(lambda: gpu.Engine(DIM, nchains=4, likelihood=gpu.LIKE_EVENT_TEMPLATE))
    refused(lambda: gpu.Engine(DIM, nchains=4, likelihood=like, likelihood_params=params, exact=False))
    eng = gpu.Engine(DIM, nchains=4, likelihood=like, likelihood_params=params, mode=gpu.MODE_PER_CHAIN)
    refused(lambda: eng.set_param("PERCHAIN_WAVE", 0))
    refused(lambda: eng.set_param("EXACT_ARITHMETIC", 0))

    def set_params(prm):
        prm = np.ascontiguousarray(prm, dtype=np.float64)
        eng._check(eng._lib.smcmc_set_likelihood_params(eng._h, prm.ctypes.data_as(gpu._capi._dp), prm.size))

    with pytest.raises(gpu.SmcmcError) as e:                           # the parameter rules hold on the engine too
        set_params(params[:-1])
    assert e.value.status == 1 and "exactly" in str(e.value)
    bad = params.copy(); bad[4] = bad[5] + 1.0
    with pytest.raises(gpu.SmcmcError) as e:
        set_params(bad)
    assert e.value.status == 1 and "cutVeryClose" in str(e.value)
    bad = params.copy(); bad[sref.HEAD + 4 * int(params[1]) + 1] += 1e-3
    with pytest.raises(gpu.SmcmcError) as e:
        set_params(bad)
    assert e.value.status == 1 and "symmetric" in str(e.value)
    bad = params.copy(); bad[sref.events_offset(params) + 1::6] = 0.0
    with pytest.raises(gpu.SmcmcError) as e:
        set_params(bad)
    assert e.value.status == 1 and "background" in str(e.value)
    assert eng.Start(scases.starts(oracle, 4, 5, params))              # and the engine is still good
    eng.close()


def test_fake_mcmc3_example(gpu, tmp_path):
    """examples/FakeMCMC3_amd.C (example3/FakeMCMC.C on the mirror) with a small Init(40, 40, 2.0) and a reduced length:
    five burn-ins of 200 to 1 000 steps and five legs of 200 saved steps (two seconds: the 31-dimensional chain with
    the two shape penalties does not move before its proposal has adapted, some 1 000 steps in); the last entry's LogLikelihood is the host definition at
    that entry's Accepted."""
    root = os.path.dirname(HERE)
    libdir = os.path.join(root, "root-simple-mcmc_amd", "lib")
    exe = str(tmp_path / "fake_mcmc3_amd.exe")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(root, 'include')}",
           os.path.join(root, "examples", "FakeMCMC3_amd.C"), f"-L{libdir}", "-lsmcmc_amd",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, prm_path = tmp_path / "fake3.csv", tmp_path / "params.txt"
    r = subprocess.run([exe, "40", "40", "2.0", "1000", "200", str(out), str(prm_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for length in (200, 400, 600, 800, 1000):                                   # burn-in k is k / 5 of the burn-in length
        assert "Start new burnin phase (%d steps)" % length in r.stdout
    assert r.stdout.count("Start chain ") == 5
    assert "28 histograms kept" in r.stdout                              # four each: initial, five burn-ins, midway (rewritten)
    lines = open(out).read().splitlines()
    col = {h: i for i, h in enumerate(lines[0].split(",")) if h}
    rows = [l.split(",") for l in lines[1:]]
    assert len(rows) == 1000
    params = np.loadtxt(prm_path)
    assert int(params[1]) == 50 and params[4] == 50.0 and params[5] == 100.0 and int(params[0]) > 100
    last = rows[-1]
    x = np.array([float(last[col[f"Accepted[{d}]"]]) for d in range(DIM)])
    assert float(last[col["LogLikelihood"]]) == gpu.event_shape_evaluate(params, x)
    logl = np.array([float(r_[col["LogLikelihood"]]) for r_ in rows])
    assert np.all(np.isfinite(logl)) and len(np.unique(logl)) > 10       # the chain moves
