"""sMCMC::FakeTemplateLikelihood (include/FakeTemplateLikelihood_amd.H), the C++ side of SMCMC_LIKE_EVENT_TEMPLATE, through
its host path alone: it compiles with warnings as errors, Init(40, 40, 2.0) makes a sample the parameter rules accept, and
operator() at MCTrueValues is event_template_evaluate at that point."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "root-simple-mcmc_amd", "lib")


def _build(tmp_path, source, name):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(ROOT, source), f"-L{LIBDIR}", "-lsmcmc_amd",
           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def run(smcmc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fake_template")
    exe = _build(tmp, os.path.join("tests", "cpp", "fake_template_host.C"), "fake_template_host.exe")
    prm = tmp / "params.txt"
    r = subprocess.run([exe, "40", "40", "2.0", str(prm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines() if line.strip()}
    return np.array([float(v) for v in open(prm).read().split()]), out


def test_device_params_pass_the_rules(run, smcmc):
    params, out = run
    nev, nbins = int(params[0]), int(params[1])
    assert nbins == 50 and params[4] == 1.0 and params.size == 8 + 3 * nbins + 6 * nev
    ev = params[8 + 3 * nbins:].reshape(nev, 6)
    # example2/Simulated.H: the floor of 1 000 signal events, at least as many background events BELOW 500 as signal
    # events, those at or above 500 kept in the sample beside them
    assert int(out["simulated"][0]) == nev and int(out["simulated"][2]) == 1000 == int(np.sum(ev[:, 1] == 0))
    assert int(out["simulated"][4]) == 1000 == int(np.sum((ev[:, 1] > 0) & (ev[:, 0] < 500.0)))
    assert np.sum(ev[:, 1] > 0) > 1000
    assert params[8:8 + 3 * nbins].sum() == 80.0                       # the 40 + 40 data events, all inside [0, 500)
    smcmc.event_template_evaluate(params, np.zeros(9))                 # (raises if a rule refuses the array)


def test_operator_at_the_true_values_is_the_host_definition(run, smcmc):
    params, out = run
    assert [float(v) for v in out["true"][:2]] == [40.0, 40.0] and int(out["true"][3]) == 9
    point = np.zeros(9)
    point[0], point[1] = 40.0, 40.0
    logl, hist, parts = smcmc.event_template_evaluate(params, point, histograms=True, parts=True)
    assert float(out["logl"][0]) == logl
    assert [float(v) for v in out["integrals"][:2]] == [parts["IS"], parts["IB"]]
    assert [float(v) for v in out["integrals"][3:5]] == [parts["ws"], parts["wb"]]
    total = 0.0
    for h in range(3):
        s = 0.0
        for v in hist[h]:
            s += v
        total = s if h == 0 else total + s
    assert float(out["expectation"][0]) == total and abs(total - 80.0) < 1e-9     # each class scaled to its count
    assert int(out["written"][0]) == 3


def test_example_compiles(smcmc, tmp_path):
    """examples/FakeMCMC2_amd.C builds against the library, warnings as errors"""
    _build(tmp_path, os.path.join("examples", "FakeMCMC2_amd.C"), "fake_mcmc2_amd.exe")
