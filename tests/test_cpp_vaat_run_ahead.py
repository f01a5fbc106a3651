"""include/TProposeVAATStep_amd.H with SetRunAhead: the caller's Step loop served from a recorded launch writes the same
tree and prints the same getters, byte for byte, as Step() one launch at a time -- through a setter
(SetAcceptanceRigidity after step 11), UpdateProposal() on a queue that is not empty (after step 17) and on an empty one
(after Start; after step 21 at dim 7), GetAcceptedAll after step 29, and SetRunAhead(false) in mid-run -- and chain 0's
columns are the reference chain's."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "root-simple-mcmc_amd", "lib")
NSTEPS = 40


def _build(tmp_path):
    exe = str(tmp_path / "vaat_run_ahead.exe")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(ROOT, "tests", "cpp", "vaat_run_ahead.C"), f"-L{LIBDIR}", "-lsmcmc_amd",
           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_driver_compiles_and_fails_loudly_without_gpu(smcmc, tmp_path):
    import torch
    exe = _build(tmp_path)
    if torch.cuda.is_available():
        return                                                       # the GPU case below runs it
    r = subprocess.run([exe, "7", "0", "1", str(tmp_path / "o.csv")], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device" in r.stderr         # no host fallback


def _mean(v):
    s = 0.0
    for a in v:                                                      # std::accumulate in index order (:160, 170)
        s += a
    return s / len(v)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,kind", [(7, 0), (64, 1)])
def test_run_ahead_writes_the_same_tree(gpu, oracle, tmp_path, dim, kind):
    exe = _build(tmp_path)
    outs = {}
    for mode in (0, 1, 2):
        out = tmp_path / f"vaat{mode}.csv"
        r = subprocess.run([exe, str(dim), str(kind), str(mode), str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"entries {NSTEPS + 1} " in r.stdout and f"likelihoods {NSTEPS + 1} " in r.stdout
        assert "agrees" in r.stdout
        outs[mode] = (open(out, "rb").read(), r.stdout)
    for mode in (1, 2):
        assert outs[0][0] == outs[mode][0], f"the tree of mode {mode} differs from the tree with the run-ahead off"
        assert outs[0][1] == outs[mode][1], (mode, outs[0][1], outs[mode][1])

    lines = outs[1][0].decode().splitlines()
    col = {h: i for i, h in enumerate(lines[0].split(",")) if h}
    rows = [l.split(",") for l in lines[1:]]
    printed = [l.split() for l in outs[1][1].splitlines() if l.startswith("step ")]
    assert len(rows) == NSTEPS + 1 and len(printed) == NSTEPS
    o = oracle.Vaat(1, dim, kind=kind, seed=20240607)
    o.set_step_rms_window(1000)                                      # TSimpleMCMC's default (:586)
    start = np.array([0.125 * (i % 5) - 0.25 for i in range(dim)])
    assert o.start(start)
    o.set_acceptance_window(20.0)
    o.update_proposal()
    for k, row in enumerate(rows):
        if k > 0:
            o.step(1)
            p = printed[k - 1]
            assert int(p[1]) == k
            assert float(p[3]) == _mean(o.per_dim("sigma")[:, 0]), k
            assert float(p[5]) == _mean(o.per_dim("acceptance")[:, 0]), k
            assert p[7] == f"{o.lane('successes')[0]}/{o.lane('trials')[0]}", k
            assert float(p[9]) == o.lane("logl_proposed")[0], k
        got = np.array([float(row[col[f"Accepted[{d}]"]]) for d in range(dim)])
        assert np.array_equal(got, o.x[:, 0]), k
        assert float(row[col["LogLikelihood"]]) == o.lane("logl")[0], k
        assert float(row[col["StepRMS"]]) == o.lane("step_rms")[0], k
        assert int(row[col["TotalSteps"]]) == k, k
        if k == 11:
            o.set_acceptance_rigidity(0.7)
        if k in (17, 21):
            o.update_proposal()
    assert o.lane("naccept")[0] > 0
