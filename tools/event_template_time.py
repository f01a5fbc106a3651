#!/usr/bin/env python3
"""Timing of SMCMC_LIKE_EVENT_TEMPLATE at example2's own size (example2/FakeLikelihood.H Init(1000, 1000, 10): 10 000 signal
events and as many background events as it takes to have 20 000 below 500, three histograms of 50 bins) beside
SMCMC_LIKE_EVENT_SAMPLE on the same sample, recorded in profiles/event_template_notes.md:
  * the pooled ensemble (step_kernel<15, ...>, one chain per lane) at 16 384 chains, ms per step of the launch;
  * one chain in SMCMC_MODE_PER_CHAIN (perchain_wave_kernel, the events dealt over the 64 lanes), us per step.
Measured as tools/event_sample_time.py measures: --warmup launches first, then the least and the median of --reps launches
timed between two device events on the engine's stream.  The two likelihoods alternate, so that a drift of the clocks
shows in both.
usage: python tools/event_template_time.py [--reps 5] [--json profiles/event_template_time.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from event_sample_time import timed  # noqa: E402


def toy_sample(pkg, data_signal=1000, data_background=1000, oversample=10.0, nbins=50, seed=1):
    """example2/Simulated.H's two populations (the background loop counts only masses below 500) and a data set drawn
    from the same populations; exposure ratio 1, as SMCMC_LIKE_EVENT_TEMPLATE demands"""
    rng = np.random.default_rng(seed)

    def positive(mean, sigma):
        m = rng.normal(mean, sigma)
        bad = m <= 0
        while bad.any():
            m[bad] = rng.normal(mean[bad], sigma[bad])
            bad = m <= 0
        return m

    def signal(n):
        tm = np.full(n, 135.0)
        return np.stack([positive(tm, 0.3 * tm), np.zeros(n), rng.exponential(150.0, n),
                         (rng.uniform(size=n) < 0.05).astype(np.float64), tm, 0.3 * tm], axis=1)

    def background(n):
        tm = rng.uniform(0.0, 1000.0, n)
        return np.stack([positive(tm, 0.4 * tm), np.ones(n), np.abs(rng.normal(0.0, 70.0, n)),
                         (rng.uniform(size=n) < 0.5).astype(np.float64), tm, 0.4 * tm], axis=1)

    ns = max(int(oversample * data_signal), 1000)
    nb = max(int(2 * oversample * data_background), ns)
    bkg = background(3 * nb)
    last = np.flatnonzero(np.cumsum(bkg[:, 0] < 500.0) == nb)[0]        # the event that completes the count
    ev = np.concatenate([signal(ns), bkg[:last + 1]])
    toy = np.concatenate([signal(data_signal), background(3 * data_background)])
    toy = toy[toy[:, 0] < 500.0][:data_signal + data_background]
    data = np.zeros((3, nbins))
    for m, _, s, k, _, _ in toy:
        data[2 if k > 0 else (0 if s < 100.0 else 1), int(nbins * m / 500.0)] += 1.0
    return pkg.event_sample_params(ev, data, nbins, 0.0, 500.0, exposure_ratio=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=4, help="steps per timed ensemble launch")
    ap.add_argument("--chain-steps", type=int, default=64, help="steps per timed launch of the single chain")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "event_template_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    params = toy_sample(pkg)
    nev, nbins = int(params[0]), int(params[1])
    nsig = int(np.sum(params[8 + 3 * nbins:].reshape(nev, 6)[:, 1] == 0))
    start = {pkg.LIKE_EVENT_SAMPLE: np.zeros(9), pkg.LIKE_EVENT_TEMPLATE: np.array([1000.0, 1000.0] + [0.0] * 7)}
    names = {pkg.LIKE_EVENT_SAMPLE: "SMCMC_LIKE_EVENT_SAMPLE", pkg.LIKE_EVENT_TEMPLATE: "SMCMC_LIKE_EVENT_TEMPLATE"}
    stream = torch.cuda.current_stream()
    rows = []
    for case, chains, mode, steps in (("pooled ensemble", a.chains, pkg.MODE_POOLED, a.steps),
                                      ("one chain, SMCMC_MODE_PER_CHAIN", 1, pkg.MODE_PER_CHAIN, a.chain_steps)):
        engines = {}
        for like in names:
            e = pkg.Engine(9, chains, likelihood=like, likelihood_params=params, mode=mode, stream=stream.cuda_stream)
            assert e.Start(start[like])
            engines[like] = e
        for repeat in range(2):                     # each likelihood twice, alternating: the run-to-run spread
            for like, e in engines.items():
                lo, med = timed(torch, stream, lambda: e.Step(steps), a.warmup if repeat == 0 else 1, a.reps)
                rows.append({"case": case, "likelihood": names[like], "repeat": repeat, "chains": chains, "steps_per_launch": steps,
                             "ms_min": lo, "ms_median": med, "us_per_step": lo * 1e3 / steps})
                print(json.dumps(rows[-1]), flush=True)
        for e in engines.values():
            e.close()
    out = dict(device=torch.cuda.get_device_name(0), nevents=nev, nsignal=nsig, nbins=nbins, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
