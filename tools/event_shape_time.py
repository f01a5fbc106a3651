#!/usr/bin/env python3
"""Timing of SMCMC_LIKE_EVENT_SHAPE at example3's own size (example3/FakeMCMC.C: Init(10000, 100, 10.0) -- 100 000 signal
events and, by the floors of example3/Simulated.H, as many background events as it takes to have 100 000 below 500; four
histograms of 50 bins) beside SMCMC_LIKE_EVENT_TEMPLATE on the same events with three histograms, recorded in
profiles/event_shape_notes.md:
  * the pooled ensemble (step_kernel<31, ...> against step_kernel<15, ...>, one chain per lane) at 2 048, 4 096, 8 192 and
    16 384 chains, ms per step of the launch;
  * one chain in SMCMC_MODE_PER_CHAIN (perchain_wave_kernel, the events dealt over the 64 lanes), ms per step.
Measured as tools/event_template_time.py measures: two warm-up launches, then the least (and the median) of five launches
timed between two device events on the engine's stream; each figure taken twice, the two likelihoods alternating.
usage: python tools/event_shape_time.py [--reps 5] [--json profiles/event_shape_time.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from event_sample_time import timed  # noqa: E402
from event_template_time import toy_sample  # noqa: E402


def shape_sample(pkg, template_params):
    """the template's events and header under SMCMC_LIKE_EVENT_SHAPE's: its Close histogram of data shared between
    VeryClose and Close, example3's kernels"""
    nev, nbins = int(template_params[0]), int(template_params[1])
    data3 = template_params[8:8 + 3 * nbins].reshape(3, nbins)
    very_close = np.floor(0.5 * data3[0])
    data4 = np.stack([very_close, data3[0] - very_close, data3[1], data3[2]])
    events = template_params[8 + 3 * nbins:].reshape(nev, 6)
    return pkg.event_shape_params(events, data4, nbins, float(template_params[2]), float(template_params[3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chains", type=int, nargs="+", default=[2048, 4096, 8192, 16384])
    ap.add_argument("--steps", type=int, default=1, help="steps per timed ensemble launch")
    ap.add_argument("--chain-steps", type=int, default=8, help="steps per timed launch of the single chain")
    ap.add_argument("--data-signal", type=int, default=10000)
    ap.add_argument("--data-background", type=int, default=100)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "event_shape_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    template = toy_sample(pkg, a.data_signal, a.data_background, 10.0)
    shape = shape_sample(pkg, template)
    nev, nbins = int(template[0]), int(template[1])
    nsig = int(np.sum(template[8 + 3 * nbins:].reshape(nev, 6)[:, 1] == 0))
    counts = [float(a.data_signal), float(a.data_background)]
    likes = {pkg.LIKE_EVENT_TEMPLATE: ("SMCMC_LIKE_EVENT_TEMPLATE", 9, template, np.array(counts + [0.0] * 7)),
             pkg.LIKE_EVENT_SHAPE: ("SMCMC_LIKE_EVENT_SHAPE", 31, shape, np.array(counts + [0.0] * 29))}
    stream = torch.cuda.current_stream()
    rows = []
    cases = [("pooled ensemble", c, pkg.MODE_POOLED, a.steps) for c in a.chains]
    cases.append(("one chain, SMCMC_MODE_PER_CHAIN", 1, pkg.MODE_PER_CHAIN, a.chain_steps))
    for case, chains, mode, steps in cases:
        engines = {}
        for like, (name, dim, params, start) in likes.items():
            e = pkg.Engine(dim, chains, likelihood=like, likelihood_params=params, mode=mode, stream=stream.cuda_stream)
            assert e.Start(start)
            engines[like] = e
        for repeat in range(2):                     # each likelihood twice, alternating: the run-to-run spread
            for like, e in engines.items():
                lo, med = timed(torch, stream, lambda: e.Step(steps), a.warmup if repeat == 0 else 1, a.reps)
                rows.append({"case": case, "likelihood": likes[like][0], "repeat": repeat, "chains": chains, "steps_per_launch": steps,
                             "ms_min": lo, "ms_median": med, "ms_per_step": lo / steps})
                print(json.dumps(rows[-1]), flush=True)
        for e in engines.values():
            e.close()
    out = dict(device=torch.cuda.get_device_name(0), nevents=nev, nsignal=nsig, nbins=nbins,
               packed_bytes={"SMCMC_LIKE_EVENT_TEMPLATE": 8 * (16 + 3 * nbins + 6 * nev),
                             "SMCMC_LIKE_EVENT_SHAPE": 8 * (16 + 4 * nbins + 314 + 8 * nev)}, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
