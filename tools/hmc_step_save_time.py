"""What an HMC trace costs, in the benchmark's HMC shape (quadratic form, D = 500, 8 192 chains, fused order, step
length fixed, 20 leapfrog steps, 64 steps per call), on the GPU box:

    python tools/hmc_step_save_time.py [--library path/to/libsmcmc_amd.so] [--repeats 5] [--steps 64]
                                       [--likelihood quad|iso] [--dim D] [--chains N] [--exact]

(the default shape runs hmc_mfma_kernel<4, true>, whose trace is the cut launch; --dim 100 runs hmc_mfma_kernel<1, true>
and --likelihood iso hmc_step_kernel, which write their slots from the one launch)

Three figures per repeat, each the median over the repeats at the end, as one JSON line:
  step_ms        Step(steps): the plain launch (compare a library of the parent commit with --library: it must not move)
  loop_ms        the trace as it was made before: `steps` x (Step(1) + copy_positions), one launch and one copy per slot
  step_save_ms   StepSave(steps, stride 1); absent for a library without smcmc_hmc_step_save
Every timing is taken between stream synchronisations after one untimed call of the same kind."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("smcmc_hmc_step_save", "smcmc_hmc_record_stride", "smcmc_hmc_step_recorded", "smcmc_hmc_snapshot",
               "smcmc_hmc_rollback")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=None, help="a build of another commit to time instead of the in-tree library")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--dim", type=int, default=500)
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--leapfrog", type=int, default=20)
    ap.add_argument("--likelihood", choices=("quad", "iso"), default="quad")
    ap.add_argument("--exact", action="store_true", help="reference-order arithmetic instead of the fused order")
    args = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    lib = pkg.load(args.library, optional=NEW_SYMBOLS)
    has_save = hasattr(lib, "smcmc_hmc_step_save")
    rng = np.random.default_rng(3)
    a = rng.standard_normal((args.dim, args.dim)) / np.sqrt(args.dim)
    err = np.linalg.inv(a @ a.T + np.eye(args.dim))
    quad = args.likelihood == "quad"
    e = pkg.HmcEngine(args.dim, args.chains, likelihood=pkg.LIKE_QUADFORM if quad else pkg.LIKE_ISO_GAUSS,
                      likelihood_params=err if quad else None, exact=args.exact or not quad, library=args.library)
    e.Start(np.full(args.dim, 0.5))
    e.SetMeanEpsilon(-0.05)
    e.SetLeapFrog(args.leapfrog)
    trace = torch.zeros((args.steps, args.dim, e.nchains_padded), dtype=torch.float64, device="cuda")
    logl = torch.zeros((args.steps, e.nchains_padded), dtype=torch.float64, device="cuda")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def loop():
        for s in range(args.steps):
            e.Step(1)
            e.copy_positions(trace[s].data_ptr())

    rows = {"step_ms": [], "loop_ms": [], "step_save_ms": []}
    for _ in range(args.repeats):
        rows["step_ms"].append(timed(lambda: e.Step(args.steps)))
        rows["loop_ms"].append(timed(loop))
        if has_save:
            rows["step_save_ms"].append(timed(lambda: e.StepSave(args.steps, trace.data_ptr(), logl.data_ptr(), stride=1)))
    out = {"library": args.library or "in-tree", "dim": args.dim, "chains": args.chains, "steps": args.steps,
           "leapfrog": args.leapfrog, "likelihood": args.likelihood, "exact": bool(args.exact or not quad)}
    for k, v in rows.items():
        if v:
            out[k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
