"""What the caller's own gradient costs (profiles/hmc_user_gradient_notes.md): trajectories per second of the fixed-step
HMC engine, HIP events around smcmc_hmc_step.

  headline   D = 500, 8 192 chains, L = 20, reference order, built-in QUADFORM:
             (i)   --parent-library PATH: a build of the parent commit, three runs (their spread is the noise band)
             (ii)  this library, no gradient matrix
             (iii) this library, a gradient matrix set (G = Error: the same trajectories, one more contraction per step)
  user       D = 100, 8 192 chains, L = 10: libsmcmc_amd_user_grad.so with gradient type 0 (smcmc_user_gradient_at) and
             type 3 (finite differences of the user likelihood), and the built-in QUADFORM for scale

  python tools/hmc_user_gradient_time.py [--parent-library PATH] [--out FILE.json] [--skip-user] [--cases i,ii,iii]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from smcmc_amd_loader import load_package  # noqa: E402

NEW_SYMBOLS = ("smcmc_hmc_has_gradient", "smcmc_hmc_set_gradient_matrix")


def error_matrix(dim):
    """TDummyLogLikelihood::Init(): unit variances, 0.999999 between the first and the last coordinate"""
    cov = np.eye(dim)
    cov[0, dim - 1] = cov[dim - 1, 0] = 0.999999
    err = np.linalg.inv(cov)
    return (err + err.T) / 2.0


def timed(pkg, stream, dim, chains, leapfrog, steps, warm, likelihood, params, library=None, gradient_type=0, matrix=None):
    h = pkg.HmcEngine(dim, chains, likelihood=likelihood, likelihood_params=params, stream=stream.cuda_stream, library=library)
    h.Start(np.ones(dim))
    h.SetMeanEpsilon(-0.001)       # the stiff pair has curvature ~1e6: a fixed step stays below 2e-3
    h.SetLeapFrog(leapfrog)
    h.SetGradientType(gradient_type)
    if matrix is not None:
        h.SetGradientMatrix(matrix)
    h.Step(warm)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream); h.Step(steps); b.record(stream)
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    accepted = float(h.lane("naccept").mean()) / (warm + steps)
    h.close()
    return {"ms_per_step": ms, "trajectories_per_s": chains / (ms * 1e-3), "accept_rate": accepted}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-library", help="libsmcmc_amd.so of the parent commit: case (i)")
    ap.add_argument("--out", help="write the rows as JSON")
    ap.add_argument("--skip-user", action="store_true")
    ap.add_argument("--cases", default="i,ii,iii", help="headline cases to run (a profiler wants one per process)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8, help="timed steps per run, after two warm-up steps")
    a = ap.parse_args()
    cases = a.cases.split(",")
    pkg = load_package()
    stream = torch.cuda.Stream()
    rows = []

    def row(name, **r):
        r = dict(case=name, **r)
        rows.append(r)
        print(json.dumps(r), flush=True)

    dim, chains, leap = 500, 8192, 20
    err = error_matrix(dim)
    if a.parent_library and "i" in cases:
        # the parent's library lacks the two new entry points: bind it without them
        pkg.load(a.parent_library, optional=NEW_SYMBOLS)
        for k in range(a.runs):
            row("(i) parent, built-in QUADFORM", run=k, dim=dim, chains=chains, leapfrog=leap,
                **timed(pkg, stream, dim, chains, leap, a.steps, 2, pkg.LIKE_QUADFORM, err, library=a.parent_library))
    for k in range(a.runs if "ii" in cases else 0):
        row("(ii) this commit, no gradient matrix", run=k, dim=dim, chains=chains, leapfrog=leap,
            **timed(pkg, stream, dim, chains, leap, a.steps, 2, pkg.LIKE_QUADFORM, err))
    for k in range(a.runs if "iii" in cases else 0):
        row("(iii) this commit, gradient matrix set", run=k, dim=dim, chains=chains, leapfrog=leap,
            **timed(pkg, stream, dim, chains, leap, a.steps, 2, pkg.LIKE_QUADFORM, err, matrix=err))
    if not a.skip_user:
        dim, leap = 100, 10
        err = error_matrix(dim)
        two = np.concatenate([err.ravel(), err.ravel()])
        grad_lib = os.path.join(ROOT, "root-simple-mcmc_amd", "lib", "libsmcmc_amd_user_grad.so")
        row("user library, gradient type 0 (smcmc_user_gradient_at)", dim=dim, chains=chains, leapfrog=leap,
            **timed(pkg, stream, dim, chains, leap, a.steps, 2, pkg.LIKE_USER, two, library=grad_lib, gradient_type=0))
        row("user library, gradient type 3 (finite differences)", dim=dim, chains=chains, leapfrog=leap,
            **timed(pkg, stream, dim, chains, leap, 2, 1, pkg.LIKE_USER, two, library=grad_lib, gradient_type=3))
        row("built-in QUADFORM", dim=dim, chains=chains, leapfrog=leap,
            **timed(pkg, stream, dim, chains, leap, a.steps, 2, pkg.LIKE_QUADFORM, err))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
