"""sMCMC::TFakeGP and sMCMC::FakeShapeLikelihood (include/TFakeGP_amd.H, include/FakeShapeLikelihood_amd.H), the C++ side
of SMCMC_LIKE_EVENT_SHAPE, through their host paths alone: they compile with warnings as errors, Init(40, 40, 2.0) makes a
sample the parameter rules accept, and TFakeGP::GetValue / GetPenalty and operator() agree with the C entry point bit for
bit."""
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "root-simple-mcmc_amd", "lib")
_spec = importlib.util.spec_from_file_location("smcmc_event_shape_ref", os.path.join(ROOT, "tests", "event_shape_ref.py"))
sref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sref)

XS = [5.0, 22.727272727272727, 100.0, 135.0, 240.0, 249.0, 260.0, 477.27272727272725, 480.0, 600.0]


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
    tmp = tmp_path_factory.mktemp("fake_shape")
    exe = _build(tmp, os.path.join("tests", "cpp", "fake_shape_host.C"), "fake_shape_host.exe")
    prm = tmp / "params.txt"
    r = subprocess.run([exe, "40", "40", "2.0", str(prm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines() if line.strip()}
    return np.array([float(v) for v in open(prm).read().split()]), out


def test_device_params_pass_the_rules(run, smcmc):
    params, out = run
    f = sref.split(params)
    nev, nbins, ev = f["nev"], f["nbins"], f["ev"]
    assert nbins == 50 and params.size == 12 + 4 * nbins + 290 + 6 * nev
    assert list(params[2:12]) == [0.0, 500.0, 50.0, 100.0, 0.05, 0.5, 0.0, 500.0, 0.0, 250.0]
    # example3/Simulated.H: the floor of 1 000 signal events, at least as many background events BELOW 500 as signal
    # events, those at or above 500 kept in the sample beside them
    assert int(out["simulated"][0]) == nev and int(out["simulated"][2]) == 1000 == int(np.sum(ev[:, 1] == 0))
    assert int(out["simulated"][4]) == 1000 == int(np.sum((ev[:, 1] > 0) & (ev[:, 0] < 500.0)))
    assert np.sum(ev[:, 1] > 0) > 1000
    assert f["data"].sum() == 80.0 and np.all(f["data"].reshape(4, nbins).sum(axis=1) > 0)    # four data histograms
    # the two kernels are example3's (libm's exp on both sides: to an ulp)
    kb, ks = sref.example3_kernels()
    assert np.allclose(f["KB"], kb, rtol=4e-16, atol=0) and np.allclose(f["KS"], ks, rtol=4e-16, atol=0)
    smcmc.event_shape_evaluate(params, np.zeros(31))                   # (raises if a rule refuses the array)


def test_operator_is_the_host_definition(run, smcmc):
    params, out = run
    assert [float(v) for v in out["true"][:2]] == [40.0, 40.0] and int(out["true"][3]) == 31
    true = np.zeros(31)
    true[0], true[1] = 40.0, 40.0
    assert float(out["logl_true"][0]) == smcmc.event_shape_evaluate(params, true)
    point = np.array([float(v) for v in out["point"]])
    assert point.size == 31 and np.all(point[9:] != 0.0) or np.count_nonzero(point[9:]) > 15
    logl, hist, parts = smcmc.event_shape_evaluate(params, point, histograms=True, parts=True)
    assert float(out["logl"][0]) == logl
    assert [float(v) for v in out["integrals"][:2]] == [parts["IS"], parts["IB"]]
    assert [float(v) for v in out["integrals"][3:5]] == [parts["ws"], parts["wb"]]
    assert [float(v) for v in out["penalties"][:2]] == [parts["penB"], parts["penS"]]
    assert int(out["written"][0]) == 4


def test_tfakegp_is_the_c_entry_point(run, smcmc):
    params, out = run
    point = np.array([float(v) for v in out["point"]])
    _, parts = smcmc.event_shape_evaluate(params, point, parts=True)
    # GetPenalty of the two shapes after operator() set them: the likelihood's own two penalties
    assert [float(v) for v in out["penalties"][3:5]] == [parts["penB"], parts["penS"]]
    yb, ys = sref.control_values([float(v) for v in point])
    lib = smcmc.load()
    C = smcmc._capi.C

    def value(low, high, y, x):
        y = np.ascontiguousarray(y, dtype=np.float64)
        v = C.c_double(0.0)
        assert lib.smcmc_event_shape_gp_value(low, high, len(y), y.ctypes.data_as(smcmc._capi._dp), x, C.byref(v)) == 0
        return v.value

    assert [float(v) for v in out["values_b"]] == [value(0.0, 500.0, yb, x) for x in XS]
    assert [float(v) for v in out["values_s"]] == [value(0.0, 250.0, ys, x) for x in XS]
    # ... which is the restatement's rule (tests/event_shape_ref.py), clamps and centres included
    assert [float(v) for v in out["values_b"]] == [sref.shape(x, yb, 0.0, 500.0)[0] for x in XS]
    assert [float(v) for v in out["values_s"]] == [sref.shape(x, ys, 0.0, 250.0)[0] for x in XS]
    assert float(out["values_s"][6]) == 0.0 and float(out["values_b"][9]) == yb[10]      # beyond the range: the end value
    # the penalty entry point by itself, and its inverse
    kb = np.ascontiguousarray(sref.split(params)["KB"])
    pen, inv = C.c_double(0.0), np.zeros((11, 11))
    y = np.ascontiguousarray(yb, dtype=np.float64)
    assert lib.smcmc_event_shape_gp_penalty(kb.ctypes.data_as(smcmc._capi._dp), 11, y.ctypes.data_as(smcmc._capi._dp), C.byref(pen),
                                            inv.ctypes.data_as(smcmc._capi._dp)) == 0
    assert pen.value == parts["penB"] and np.array_equal(inv, parts["KinvB"])
    bad = kb.copy(); bad[0, 1] += 1e-3
    assert lib.smcmc_event_shape_gp_penalty(bad.ctypes.data_as(smcmc._capi._dp), 11, y.ctypes.data_as(smcmc._capi._dp), C.byref(pen),
                                            None) == 1
    assert b"symmetric" in lib.smcmc_event_sample_last_error()
    # the small members
    b = out["bins"]
    assert [float(b[0]), float(b[1])] == [11.0, 13.0]
    assert float(b[3]) == sref.centres(0.0, 500.0, 11)[3] and float(b[4]) == sref.centres(0.0, 250.0, 13)[12]
    assert float(b[6]) == yb[4] and float(b[7]) == 0.0
    kb3, ks3 = sref.example3_kernels()
    assert float(b[9]) == pytest.approx(kb3[2, 5], rel=4e-16) and float(b[10]) == pytest.approx(ks3[12, 0], rel=4e-16)
    e = [float(v) for v in out["exponential"]]
    assert e[0] == 9.0 and e[1] == 0.0 and e[2] == 0.0                  # |r| = 22.7 > 20 -> exactly 0


def test_example_compiles(smcmc, tmp_path):
    """examples/FakeMCMC3_amd.C builds against the library, warnings as errors"""
    _build(tmp_path, os.path.join("examples", "FakeMCMC3_amd.C"), "fake_mcmc3_amd.exe")
