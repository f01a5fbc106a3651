#!/usr/bin/env python3
"""Timing of the lag-grid autocorrelation sums (smcmc_autocorrelation_grid_sums: autocorr_grid_partial_kernel, one
launch whose grid z is the passes of 32 lags, and its reduction) beside the contiguous reducer that reads the same
trace in the same process (smcmc_autocorrelation_sums: autocorr_partial_kernel<0> and <32>).

The ensemble trace is the largest of (512, 128, 32) slots x D = 50 x 65 536 chains that the card's free memory allows,
written by StepSave; the single chain is 1 chain x D = 50 x 100 000 slots of an AR(1) series (phi = 0.999, so that the
far lags are not noise), in a trace padded to 64 lanes.  Each number is the time of the whole C call between two device
events after one warm-up call (it includes the call's own allocations and copies): the median, the least and the mean
of --reps; the calls on one trace alternate, so that a drift of the machine touches all of them.
  bytes read      8 x values x (1 for a pass whose first lag is 0, else 2: u and its partner w) per pass that loads;
                  a pass whose first lag lies beyond the trace loads nothing
  multiply-adds   32 per loaded u value and pass (the register block computes all 32 lags of a pass, whether or not the
                  grid asks for them), the rate from the median
usage: python tools/autocorr_grid_time.py [--reps 7] [--json profiles/autocorr_grid_time.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS = 8.0


def grid_work(nslots, values_per_slot, lag_first, lag_step, nlags):
    """(passes that load, bytes read, multiply-adds) of one grid call, from the shapes."""
    passes = [lag_first + 32 * p * lag_step for p in range((nlags + 31) // 32)]
    values = float(nslots) * values_per_slot
    loading = [k0 for k0 in passes if k0 < nslots or k0 == passes[0]]
    nbytes = sum(8.0 * values * (1 if k0 == 0 else 2) for k0 in loading)
    return len(loading), nbytes, 32.0 * values * len(loading)


def time_calls(torch, stream, calls, reps):
    ms = {name: [] for name in calls}
    for call in calls.values():                          # warm-up: code object, allocator
        call()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, call in calls.items():                 # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--slots", type=int, nargs="+", default=[512, 128, 32], help="candidates, the largest that fits is used")
    ap.add_argument("--single-slots", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "autocorr_grid_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    rows = []

    def report(name, trace, ms, work):
        passes, nbytes, fmas = work
        med = float(np.median(ms))
        row = {"call": name, "trace": trace, "passes": passes, "bytes": nbytes, "fma": fmas, "ms_median": med,
               "ms_min": min(ms), "ms_mean": float(np.mean(ms)), "TBps_at_median": nbytes / (med * 1e-3) / 1e12,
               "Tfma_per_s_at_median": fmas / (med * 1e-3) / 1e12, "hbm_floor_ms": nbytes / (HBM_PEAK_TBPS * 1e12) * 1e3}
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- the ensemble -------------------------------------------------------------------------------------------------
    e = pkg.Engine(a.dim, a.chains, mode=pkg.MODE_POOLED, stream=st)
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
    ptr, centre = sx.data_ptr(), e.GetEstimatedCenter()
    plan = pkg.autocorrelation_plan(slots)
    macro = (1, plan.lag_step, len(plan.lags))
    calls = {"contiguous reducer, lags 0..63": lambda: e.AutocorrelationSums(ptr, slots, centre=centre, stream=st),
             "grid (0, 1, 64)": lambda: e.AutocorrelationGrid(ptr, slots, 0, 1, 64, centre=centre, stream=st),
             "grid, the macro's plan %s" % (macro,): lambda: e.MakeAutocorrelation(ptr, slots, stream=st, centre=centre)}
    ms = time_calls(torch, stream, calls, a.reps)
    per = a.dim * a.chains
    trace = "%d slots x %d x %d chains" % (slots, a.dim, a.chains)
    names = list(calls)
    report(names[0], trace, ms[names[0]], grid_work(slots, per, 0, 1, 64))
    report(names[1], trace, ms[names[1]], grid_work(slots, per, 0, 1, 64))
    report(names[2], trace, ms[names[2]], grid_work(plan.trials, per, *macro))
    same = e.AutocorrelationGrid(ptr, slots, 0, 1, 64, centre=centre, stream=st)
    old = e.AutocorrelationSums(ptr, slots, centre=centre, stream=st)
    check = {"grid_0_1_64_has_the_contiguous_bits": bool(np.array_equal(same.lagged, old.lagged) and np.array_equal(same.sum, old.sum)),
             "ratio_grid_0_1_64_over_contiguous": rows[1]["ms_median"] / rows[0]["ms_median"]}
    trace_bytes = float(slots * per_slot)
    del sx, sl
    e.close()
    torch.cuda.empty_cache()

    # ---- one chain, the macro's own case --------------------------------------------------------------------------------
    n = a.single_slots
    rng = np.random.default_rng(1)
    noise = rng.standard_normal((n, a.dim))
    x = np.zeros((n, a.dim))
    for t in range(1, n):
        x[t] = 0.999 * x[t - 1] + noise[t]
    one = torch.full((n, a.dim, 64), float("nan"), dtype=torch.float64, device="cuda")
    one[:, :, 0] = torch.from_numpy(x).to("cuda")
    torch.cuda.synchronize()
    s = pkg.HmcEngine(a.dim, 1, stream=st)               # any engine of one chain and dim_stride = dim serves the trace
    plan1 = pkg.autocorrelation_plan(n)
    macro1 = (1, plan1.lag_step, len(plan1.lags))
    name1 = "one chain, the macro's plan %s" % (macro1,)
    ms1 = time_calls(torch, stream, {name1: lambda: s.MakeAutocorrelation(one.data_ptr(), n, stream=st)}, a.reps)
    report(name1, "%d slots x %d x 1 chain" % (n, a.dim), ms1[name1], grid_work(plan1.trials, a.dim, *macro1))
    m = s.MakeAutocorrelation(one.data_ptr(), n, stream=st)
    k = plan1.lags[plan1.lag_bins == 1]
    check["one_chain_autocorr_bin1"] = float(m.average[1])
    check["one_chain_ar1_expectation_bin1"] = float(np.mean(0.999 ** k))
    print(json.dumps(check), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), hbm_peak_TBps=HBM_PEAK_TBPS, ensemble_trace_bytes=trace_bytes,
               reps=a.reps, rows=rows, check=check)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()
