#!/usr/bin/env python3
"""Timing of the device sums behind split R-hat and the multi-chain ESS (smcmc_trace_convergence: chain_sums_kernel,
within_partial_kernel<0> and <32>, ordered_rows_reduce_kernel) beside existing code that reads the same bytes in the same
process: the autocorrelation reducer (smcmc_autocorrelation_sums: autocorr_partial_kernel<0> and <32>, whose register
shape the second pass shares, and its reduction).

The trace is the largest of (512, 128, 32) slots x D = 50 x 65 536 chains that the card's free memory allows, written by
StepSave.  Each number is the time of the whole C call between two device events after one warm-up call (it includes
the call's own allocations and copies), the least and the mean of --reps; the two calls alternate, so that a drift of
the machine touches both.  The kernels alone come from `rocprofv3 --kernel-trace --stats` over this command in a run of
its own (--reps 3 is enough there): it separates the two passes and the two autocorrelation kernels.
  bytes read per pass over the trace:  8 x slots x dim x chains (the HBM floor of a pass: those bytes at the peak)
  passes:  convergence 3 (the sums, lags 0..31, lags 32..63), autocorrelation 2
usage: python tools/convergence_time.py [--reps 5] [--segments 2] [--json profiles/convergence_time.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--slots", type=int, nargs="+", default=[512, 128, 32], help="candidates, the largest that fits is used")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "convergence_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    stream = torch.cuda.current_stream()
    e = pkg.Engine(a.dim, a.chains, mode=pkg.MODE_POOLED, stream=stream.cuda_stream)
    assert e.Start(np.zeros(a.dim))
    for _ in range(4):                                   # the pooled proposal adapts: a realistic posterior sample
        e.Step(64)
        e.sync()
    free, _ = torch.cuda.mem_get_info()
    per_slot = 8 * e.dim_padded * e.nchains_padded
    slots = next((s for s in sorted(a.slots, reverse=True) if s * per_slot * 1.1 + (2 << 30) < free), None)
    if slots is None:
        raise SystemExit("no candidate trace fits the free memory (%d bytes)" % free)
    sx = torch.empty((slots, e.dim_padded, e.nchains_padded), dtype=torch.float64, device="cuda")
    sl = torch.empty((slots, e.nchains_padded), dtype=torch.float64, device="cuda")
    e.StepSave(slots * 2, sx.data_ptr(), sl.data_ptr(), stride=2)
    torch.cuda.synchronize()
    value_bytes = 8.0 * slots * a.dim * a.chains
    hbm_floor_ms = value_bytes / (HBM_PEAK_TBPS * 1e12) * 1e3
    ptr, st = sx.data_ptr(), stream.cuda_stream
    centre = e.GetEstimatedCenter()
    calls = {"convergence (3 passes + reduction)": (3, lambda: e.Convergence(ptr, slots, nsegments=a.segments, centre=centre, stream=st)),
             "autocorrelation (2 passes + reduction)": (2, lambda: e.AutocorrelationSums(ptr, slots, centre=centre, stream=st))}
    ms = {name: [] for name in calls}
    for _, call in calls.values():                       # warm-up: code object, allocator
        call()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for name, (_, call) in calls.items():            # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    rows = []
    for name, (passes, _) in calls.items():
        row = {"call": name, "slots": slots, "dim": a.dim, "chains": a.chains, "segments": a.segments, "passes": passes,
               "bytes": passes * value_bytes, "ms_min": min(ms[name]), "ms_mean": float(np.mean(ms[name])),
               "TBps_at_min": passes * value_bytes / (min(ms[name]) * 1e-3) / 1e12, "hbm_floor_ms": passes * hbm_floor_ms}
        rows.append(row)
        print(json.dumps(row), flush=True)
    # what was timed, as a sanity check: the split R-hat and tau of the trace beside the pooled estimator's tau
    c = e.Convergence(ptr, slots, nsegments=a.segments, centre=centre, stream=st)
    pooled = e.AutocorrelationSums(ptr, slots, centre=centre, stream=st)
    check = {"rhat_max": float(np.max(c.rhat())), "tau_median": float(np.median(c.tau())),
             "pooled_tau_median": float(np.median(pooled.tau())), "truncated_dims": int(np.sum(c.truncated()))}
    print(json.dumps(check), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), hbm_peak_TBps=HBM_PEAK_TBPS, trace_bytes=float(slots * per_slot),
               value_bytes_per_pass=value_bytes, hbm_floor_ms_per_pass=hbm_floor_ms, rows=rows, check=check)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    e.close()


if __name__ == "__main__":
    main()
