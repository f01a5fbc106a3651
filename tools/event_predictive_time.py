#!/usr/bin/env python3
"""Timing of the posterior-predictive reducer (smcmc_event_predictive_sums, Engine.PosteriorPredictive) beside the two
things it can be held against, taken in the same process on the same card, recorded in profiles/event_predictive_notes.md:
  * SMCMC_LIKE_EVENT_SAMPLE at example/'s own size (30 000 simulated events, three histograms of 50 bins;
    tools/event_sample_time.py's sample) and SMCMC_LIKE_EVENT_SHAPE at example3/'s (tools/event_shape_time.py's sample,
    four histograms of 50 bins);
  * the trace: --slots x --chains points, saved by StepSave from a pooled ensemble of that many chains started at the
    tools' own start points;
  * the reducer over it, points/s: the whole C call (it packs and uploads the sample, allocates its scratch, launches,
    reduces and copies the sums back) between two device events, without and with the histograms of every point written
    out;
  * the step kernel's chain-steps/s for the same likelihood and chain count, measured as tools/event_sample_time.py and
    tools/event_shape_time.py measure it;
  * the host evaluator's evaluations/s on one core (every call checks and packs the sample again).
Each device figure: --warmup calls first, then the least and the median of --reps calls.
usage: python tools/event_predictive_time.py [--reps 3] [--json profiles/event_predictive_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from event_sample_time import timed, toy_sample as sample_toy  # noqa: E402
from event_shape_time import shape_sample  # noqa: E402
from event_template_time import toy_sample as template_toy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--members", nargs="+", default=["sample", "shape"], choices=["sample", "shape"])
    ap.add_argument("--host-seconds", type=float, default=2.0)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "event_predictive_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    stream = torch.cuda.current_stream()
    members = {}
    if "sample" in a.members:
        members["SMCMC_LIKE_EVENT_SAMPLE"] = (pkg.LIKE_EVENT_SAMPLE, 9, sample_toy(pkg), np.zeros(9), 4, pkg.event_sample_evaluate)
    if "shape" in a.members:
        shape = shape_sample(pkg, template_toy(pkg, 10000, 100, 10.0))
        members["SMCMC_LIKE_EVENT_SHAPE"] = (pkg.LIKE_EVENT_SHAPE, 31, shape, np.array([10000.0, 100.0] + [0.0] * 29), 1,
                                             pkg.event_shape_evaluate)
    rows = []
    for name, (like, dim, params, start, steps, evaluate) in members.items():
        nev, nbins = int(params[0]), int(params[1])
        e = pkg.Engine(dim, a.chains, likelihood=like, likelihood_params=params, mode=pkg.MODE_POOLED, stream=stream.cuda_stream)
        assert e.Start(start)
        npad, stride = e.nchains_padded, e.dim_padded
        sx = torch.empty((a.slots, stride, npad), dtype=torch.float64, device="cuda")
        sl = torch.empty((a.slots, npad), dtype=torch.float64, device="cuda")
        e.StepSave(a.slots, sx.data_ptr(), sl.data_ptr(), stride=1)
        torch.cuda.synchronize()
        points = a.slots * a.chains
        base = {"likelihood": name, "nevents": nev, "nbins": nbins, "slots": a.slots, "chains": a.chains}

        lo, med = timed(torch, stream, lambda: e.Step(steps), 2, 5)
        rows.append(dict(base, case="step kernel, pooled ensemble", steps_per_launch=steps, ms_min=lo, ms_median=med,
                         chain_steps_per_s=a.chains * steps / (lo * 1e-3)))
        print(json.dumps(rows[-1]), flush=True)

        ptr, st = sx.data_ptr(), stream.cuda_stream
        first = e.PosteriorPredictive(ptr, a.slots, stream=st)
        centre = np.where(np.isfinite(first.mean), first.mean, 0.0)
        lo, med = timed(torch, stream, lambda: e.PosteriorPredictive(ptr, a.slots, centre=centre, stream=st), a.warmup, a.reps)
        rows.append(dict(base, case="posterior predictive, sums alone", ms_min=lo, ms_median=med, points_per_s=points / (lo * 1e-3)))
        print(json.dumps(rows[-1]), flush=True)
        rows_h = first.data.size
        hist = torch.empty((a.slots, rows_h, npad), dtype=torch.float64, device="cuda")
        logl = torch.empty((a.slots, npad), dtype=torch.float64, device="cuda")
        lo, med = timed(torch, stream, lambda: e.PosteriorPredictive(ptr, a.slots, centre=centre, histograms_ptr=hist.data_ptr(),
                                                                    logl_ptr=logl.data_ptr(), stream=st), a.warmup, a.reps)
        rows.append(dict(base, case="posterior predictive, histograms and logl of every point written", ms_min=lo, ms_median=med,
                         points_per_s=points / (lo * 1e-3), bytes_written=8.0 * a.slots * (rows_h + 1) * npad))
        print(json.dumps(rows[-1]), flush=True)
        # what was timed is what the step kernel saved
        agree = bool(torch.equal(logl[:, :a.chains], sl[:, :a.chains]))
        print(json.dumps({"likelihood": name, "recomputed logl equals the saved logl": agree}), flush=True)
        del hist, logl, sx, sl
        e.close()

        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < a.host_seconds:
            evaluate(params, start, histograms=True)
            n += 1
        rows.append(dict(base, case="host evaluator with histograms, one core (packs the sample every call)",
                         evaluations_per_s=n / (time.perf_counter() - t0), logl_agrees=agree))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
