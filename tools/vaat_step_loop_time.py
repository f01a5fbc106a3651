"""Time the unchanged caller's loop around the variable-at-a-time proposal (examples/VaatStepLoop_amd.C,
SimpleVAAT.C:47-61) with Step() one launch per call (run-ahead 0: what every Step() cost before
smcmc_vaat_step_recorded existed, the baseline) and with Step() running ahead (run-ahead 1), on the GPU:

    python tools/vaat_step_loop_time.py [--out profiles/vaat_step_loop.json] [--repeats 3]

Shapes: iso-Gaussian D = 5 and D = 50, header-form TDummyLogLikelihood D = 100 (SimpleVAAT.C's own configuration), one
chain and 64 chains, every step saved to the tree.  Every run is a process of its own under its own time limit; a run
that fails or runs out of time ends the tool.  The figure is the example's own "steps_per_s": the host clock around the
loop, whose last call ends in a read of the device."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "root-simple-mcmc_amd", "lib")
# (name, dim, likelihood, steps with the run-ahead off, steps with it on): about a second of loop each
SHAPES = [("iso-Gaussian D=5", 5, 0, 20000, 400000), ("iso-Gaussian D=50", 50, 0, 20000, 200000),
          ("SimpleVAAT.C: header-form TDummy D=100", 100, 1, 10000, 20000)]
CHAINS = (1, 64)


def build(tmp):
    exe = os.path.join(tmp, "vaat_step_loop.exe")
    cmd = ["g++", "-std=c++17", "-O2", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "examples", "VaatStepLoop_amd.C"),
           f"-L{LIBDIR}", "-lsmcmc_amd", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, dim, kind, steps, ahead, chains, limit):
    cmd = [exe, str(dim), "2", str(steps // 2), "1", str(ahead), "", str(chains), str(kind)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stdout}{r.stderr}")
    words = r.stdout.split()
    if int(words[words.index("run_ahead") + 1]) != ahead:
        raise RuntimeError(f"run-ahead {ahead} asked for, the example reports {r.stdout}")
    return float(words[words.index("steps_per_s") + 1]), int(words[words.index("entries") + 1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vaat_step_loop.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=float, default=60.0, help="seconds allowed to each run")
    a = ap.parse_args()
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, dim, kind, steps_off, steps_on in SHAPES:
            for chains in CHAINS:
                rates = {0: [], 1: []}
                for _ in range(a.repeats):            # the two alternate, so that a busy host slows both
                    for ahead, steps in ((0, steps_off), (1, steps_on)):
                        rate, entries = run(exe, dim, kind, steps, ahead, chains, a.limit)
                        assert entries == 2 * (steps // 2), entries
                        rates[ahead].append(rate)
                row = {"workload": name, "dim": dim, "chains": chains, "saved_every_step": True,
                       "steps_timed": {"run_ahead_0": steps_off, "run_ahead_1": steps_on},
                       "step_calls_per_s_run_ahead_0": rates[0], "step_calls_per_s_run_ahead_1": rates[1],
                       "median_run_ahead_0": statistics.median(rates[0]), "median_run_ahead_1": statistics.median(rates[1])}
                row["factor"] = row["median_run_ahead_1"] / row["median_run_ahead_0"]
                results.append(row)
                print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
