"""include/TSimpleHMC_amd.H with SetPerChainAdaptation(true): 64 chains through the reference's Step loop, and chain 0's
tree columns are the reference chain's (oracle.Hmc chain 0)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "root-simple-mcmc_amd", "lib")


def _build(tmp_path):
    exe = str(tmp_path / "hmc_per_chain.exe")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(ROOT, "tests", "cpp", "hmc_per_chain.C"), f"-L{LIBDIR}", "-lsmcmc_amd",
           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_mirror_compiles(smcmc, tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_mirror_per_chain_is_the_reference_chain(gpu, oracle, tmp_path):
    exe = _build(tmp_path)
    dim, nsteps = 5, 4 * 5 + 10
    out = tmp_path / "hmc.csv"
    r = subprocess.run([exe, str(dim), str(nsteps), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"entries {nsteps + 1}" in r.stdout
    lines = open(out).read().splitlines()
    header = lines[0].split(",")
    col = {h: i for i, h in enumerate(header) if h}
    rows = [l.split(",") for l in lines[1:]]
    h = oracle.Hmc(dim, seed=20240607, chain_id=0, potential_from_gradient=True)
    h.start(np.ones(dim))
    updates = 0
    for k, row in enumerate(rows):
        if k > 0:
            h.step()
        s = h.scalars
        got = np.array([float(row[col[f"Accepted[{d}]"]]) for d in range(dim)])
        assert np.array_equal(got, h.accepted), k
        assert float(row[col["LogLikelihood"]]) == s["accepted_potential"], k
        assert float(row[col["MeanEpsilon"]]) == s["mean_epsilon"], k
        assert int(row[col["Leapfrog"]]) == s["leapfrog_steps"], k
        assert float(row[col["Trace"]]) == s["trace"], k
        assert float(row[col["Orbit"]]) == s["orbit"], k
        updates = s["updates"]
    assert updates >= 1
