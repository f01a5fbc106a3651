"""Does the recording path of the variable-at-a-time kernels cost the plain smcmc_vaat_step anything?  Times
smcmc_vaat_step through two builds of the library in one process, alternating them:

    python tools/vaat_step_record_cost.py --parent <libsmcmc_amd.so of the parent commit> [--out profiles/vaat_step_record_cost.json]

Shapes: iso-Gaussian D = 50 with 65 536 chains (the shape of profiles/r02_vaat.json) and the header-form quadratic form
D = 100 with 4 096 chains; five runs of each build, parent and new in turn; a run is a fresh engine, warm-up launches,
then a window of launches between two device synchronisations on the host clock.  Both series go to the file with their
medians and the parent's own run-to-run spread, which is what the difference of the medians is judged against."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# (name, dim, likelihood, chains, steps per launch, launches in the window)
SHAPES = [("README-form TDummy (iso) D=50", 50, 0, 65536, 1000, 40),
          ("header-form TDummy (quadratic form) D=100", 100, 1, 4096, 200, 20)]
NEW_SYMBOLS = ("smcmc_vaat_record_stride", "smcmc_vaat_step_recorded", "smcmc_vaat_snapshot", "smcmc_vaat_rollback")


def one_run(pkg, torch, library, dim, kind, chains, steps, launches):
    prm = None
    if kind == 1:                       # any symmetric positive definite Error matrix times alike
        a = np.random.default_rng(3).standard_normal((dim, dim)) / np.sqrt(dim)
        prm = np.linalg.inv(a @ a.T + np.eye(dim))
    e = pkg.VaatEngine(dim, chains, likelihood=kind, likelihood_params=prm, seed=11, library=library)
    assert e.Start(np.random.default_rng(dim).uniform(-1.0, 1.0, size=(dim, chains)))
    e.UpdateProposal()
    for _ in range(3):
        e.Step(steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        e.Step(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    check = float(e.lane("logl").sum())
    e.close()
    return chains * steps * launches / dt, check


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vaat_step_record_cost.json"))
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    from root_simple_mcmc_amd import _capi
    _capi.load(a.parent, optional=NEW_SYMBOLS)
    builds = (("parent", os.path.abspath(a.parent)), ("new", None))
    results = []
    for name, dim, kind, chains, steps, launches in SHAPES:
        series = {"parent": [], "new": []}
        checks = {"parent": set(), "new": set()}
        for _ in range(a.runs):
            for tag, lib in builds:
                rate, check = one_run(pkg, torch, lib, dim, kind, chains, steps, launches)
                series[tag].append(rate)
                checks[tag].add(check)
        assert checks["parent"] == checks["new"] and len(checks["new"]) == 1, checks   # the same chains, bit for bit
        med = {t: statistics.median(series[t]) for t in series}
        row = {"workload": name, "dim": dim, "chains": chains, "steps_per_launch": steps, "launches_timed": launches,
               "chain_steps_per_s_parent": series["parent"], "chain_steps_per_s_new": series["new"],
               "median_parent": med["parent"], "median_new": med["new"],
               "new_over_parent": med["new"] / med["parent"],
               "parent_spread": (max(series["parent"]) - min(series["parent"])) / med["parent"],
               "within_parent_spread": med["new"] >= med["parent"] - (max(series["parent"]) - min(series["parent"]))}
        results.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0 if all(r["within_parent_spread"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
