"""examples/VaatStepLoop_amd.C, the caller's loop of SimpleVAAT.C:47-61 on TProposeVAATStep_amd.H: it compiles, and the
tree it writes is the same with Step() running ahead, one launch per call, and the run-ahead turned off in mid-run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "root-simple-mcmc_amd", "lib")


def _build(tmp_path):
    exe = str(tmp_path / "vaat_step_loop.exe")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(ROOT, "examples", "VaatStepLoop_amd.C"), f"-L{LIBDIR}", "-lsmcmc_amd",
           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_vaat_step_loop_driver_compiles(smcmc, tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_vaat_run_ahead_step_is_the_same_chain(gpu, tmp_path):
    exe = _build(tmp_path)
    dim, cycles, steps = 5, 3, 700
    outs = []
    for ahead in (0, 1, 2):                              # 2: run-ahead on, SetRunAhead(false) after the first cycle
        out = tmp_path / f"tree{ahead}.csv"
        r = subprocess.run([exe, str(dim), str(cycles), str(steps), "1", str(ahead), str(out)], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"run_ahead {1 if ahead == 1 else 0}" in r.stdout
        outs.append((open(out).read(), r.stdout.split("moved")[1].split("run_ahead")[0] + r.stdout.split("printed")[1]))
    assert outs[0][1] == outs[1][1] == outs[2][1]        # moved / entries / the printed getters
    assert outs[0][0] == outs[1][0] == outs[2][0]        # the trees, as text: every column of every entry
    assert len(outs[0][0].splitlines()) == cycles * steps + 1
