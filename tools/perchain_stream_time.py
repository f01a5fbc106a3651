#!/usr/bin/env python3
"""SMCMC_MODE_PER_CHAIN on the streamed one-chain-per-workgroup kernel (SMCMC_P_PERCHAIN_STREAM): chain-steps/s of the
isotropic Gaussian at D = 200 and D = 500 for 1, 64, 256 and 1 024 chains, launches of 256 steps, a warm-up and then the
median of the timed launches -- and beside each figure oracle.Chain at the same D on one host core of the same box, in
the same run.  The cost of a launch's two transpositions (tiled images <-> working copies) is what a launch of one step
takes beyond one step of the long launch.
usage: python tools/perchain_stream_time.py [--dims 200 500] [--chains 1 64 256 1024] [--steps 256] [--launches 7]
                                            [--json profiles/perchain_stream.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(e, stream, torch, steps, launches):
    """milliseconds of `launches` calls of Step(steps), by device events"""
    evs = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); e.Step(steps); e1.record(stream)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return [x.elapsed_time(y) for x, y in evs]


def oracle_rate(O, dim, steps):
    """steps/s of oracle.Chain on one core: a warm-up, then the median of five runs"""
    c = O.Chain(dim, chain_id=0)
    assert c.start(np.zeros(dim))
    c.run_quiet(steps)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        c.run_quiet(steps)
        times.append(time.perf_counter() - t0)
    return steps / float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[200, 500])
    ap.add_argument("--chains", type=int, nargs="+", default=[1, 64, 256, 1024])
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--json")
    a = ap.parse_args()
    assert a.launches >= 5
    import torch
    from smcmc_amd_loader import load_package
    from oracle import oracle as O
    O.build()
    pkg = load_package()
    stream = torch.cuda.current_stream()
    rows = []
    for dim in a.dims:
        ora = oracle_rate(O, dim, a.steps)
        for n in a.chains:
            e = pkg.Engine(dim, n, mode=pkg.MODE_PER_CHAIN, stream=stream.cuda_stream, perchain_stream=True)
            assert e.get_param("PERCHAIN_STREAM") == 1
            assert e.Start(np.zeros(dim))
            e.Step(a.steps)                                      # warm-up (the free-running schedule: updates are rare)
            torch.cuda.synchronize()
            long_ms = float(np.median(_timed(e, stream, torch, a.steps, a.launches)))
            one_ms = float(np.median(_timed(e, stream, torch, 1, a.launches)))
            step_ms = long_ms / a.steps
            rate = n * a.steps / (long_ms * 1e-3)
            rows.append({"dim": dim, "chains": n, "likelihood": "ISO", "steps_per_launch": a.steps, "launches": a.launches,
                         "ms_per_launch_median": long_ms, "us_per_ensemble_step": step_ms * 1e3,
                         "chain_steps_per_s": rate,
                         "ms_launch_of_one_step": one_ms, "ms_transpositions_and_launch": one_ms - step_ms,
                         "oracle_one_core_steps_per_s": ora, "ratio_to_one_core": rate / ora,
                         "ratio_to_16_cores": rate / (16.0 * ora),
                         "updates_per_chain": float(e.lane("update_count").mean())})
            print(json.dumps(rows[-1]), flush=True)
            e.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
