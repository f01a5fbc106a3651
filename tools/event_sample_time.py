#!/usr/bin/env python3
"""Timing of SMCMC_LIKE_EVENT_SAMPLE at the reference's own size (example/FakeLikelihood.H: 30 000 simulated events, three
histograms of 50 bins), recorded in profiles/event_sample_notes.md:
  * the pooled ensemble (step_kernel<15, EVENT_SAMPLE>, one chain per lane) at 16 384 and 65 536 chains, chain-steps/s;
  * one chain in SMCMC_MODE_PER_CHAIN (perchain_wave_kernel, the events dealt over the 64 lanes), us per step;
  * Step() calls/s of examples/FakeMCMC_amd.C through the C++ mirror (one chain, run-ahead), when --exe names the binary;
  * smcmc_event_sample_evaluate on one host core, evaluations/s (every call packs the sample again: three logarithms per
    event beside the two exponentials of the evaluation itself).
Each device figure: --warmup launches first (code object, clocks), then the least and the median of --reps launches timed
between two device events on the engine's stream.
usage: python tools/event_sample_time.py [--reps 5] [--exe fake_mcmc_amd.exe] [--json profiles/event_sample_time.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def toy_sample(pkg, nsignal=10000, nbackground=20000, nbins=50, seed=1):
    """Simulated.H's two populations and a data set of a tenth of the size from the same populations."""
    rng = np.random.default_rng(seed)

    def population(ns, nb):
        def positive(mean, sigma):
            m = rng.normal(mean, sigma)
            bad = m <= 0
            while bad.any():
                m[bad] = rng.normal(mean[bad], sigma[bad])
                bad = m <= 0
            return m
        tm = np.concatenate([np.full(ns, 135.0), rng.uniform(0.0, 1000.0, nb)])
        sg = 0.3 * tm
        mass = positive(tm, sg)
        typ = np.concatenate([np.zeros(ns), np.ones(nb)])
        sep = np.concatenate([rng.exponential(100.0, ns), np.abs(rng.normal(0.0, 50.0, nb))])
        mudk = np.concatenate([rng.uniform(size=ns) < 0.05, rng.uniform(size=nb) < 0.5]).astype(np.float64)
        return np.stack([mass, typ, sep, mudk, tm, sg], axis=1)
    ev = population(nsignal, nbackground)
    toy = population(nsignal // 10, nbackground // 10)
    data = np.zeros((3, nbins))
    for m, _, s, k, _, _ in toy:
        if 0.0 <= m < 500.0:
            data[2 if k > 0 else (0 if s < 100.0 else 1), int(nbins * m / 500.0)] += 1.0
    return pkg.event_sample_params(ev, data, nbins, 0.0, 500.0)


def timed(torch, stream, call, warmup, reps):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4, help="steps per timed ensemble launch")
    ap.add_argument("--chain-steps", type=int, default=64, help="steps per timed launch of the single chain")
    ap.add_argument("--exe", default=None, help="examples/FakeMCMC_amd.C built: its Step() rate is recorded too")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "event_sample_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    params = toy_sample(pkg)
    rows = []
    stream = torch.cuda.current_stream()
    for chains in (16384, 65536):
        e = pkg.Engine(9, chains, likelihood=pkg.LIKE_EVENT_SAMPLE, likelihood_params=params, mode=pkg.MODE_POOLED,
                       stream=stream.cuda_stream)
        assert e.Start(np.zeros(9))
        lo, med = timed(torch, stream, lambda: e.Step(a.steps), a.warmup, a.reps)
        rows.append({"case": "pooled ensemble", "chains": chains, "steps_per_launch": a.steps, "ms_min": lo, "ms_median": med,
                     "chain_steps_per_s": chains * a.steps / (lo * 1e-3)})
        print(json.dumps(rows[-1]), flush=True)
        e.close()
    e = pkg.Engine(9, 1, likelihood=pkg.LIKE_EVENT_SAMPLE, likelihood_params=params, mode=pkg.MODE_PER_CHAIN,
                   stream=stream.cuda_stream)
    assert e.Start(np.zeros(9))
    lo, med = timed(torch, stream, lambda: e.Step(a.chain_steps), a.warmup, a.reps)
    rows.append({"case": "one chain, SMCMC_MODE_PER_CHAIN", "steps_per_launch": a.chain_steps, "ms_min": lo, "ms_median": med,
                 "us_per_step": lo * 1e3 / a.chain_steps})
    print(json.dumps(rows[-1]), flush=True)
    e.close()
    if a.exe:
        r = subprocess.run([a.exe, "1000", "1000", "10.0", os.devnull], capture_output=True, text=True, timeout=900)
        rate = [l for l in r.stdout.splitlines() if l.startswith("steps_per_s")]
        rows.append({"case": "Step() through the C++ mirror (examples/FakeMCMC_amd.C)", "returncode": r.returncode,
                     "steps_per_s": float(rate[0].split()[1]) if rate else None})
        print(json.dumps(rows[-1]), flush=True)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < 2.0:
        pkg.event_sample_evaluate(params, np.zeros(9))
        n += 1
    rows.append({"case": "smcmc_event_sample_evaluate, one host core (packs the sample every call)",
                 "evaluations_per_s": n / (time.perf_counter() - t0)})
    print(json.dumps(rows[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), nevents=int(params[0]), nbins=int(params[1]), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
