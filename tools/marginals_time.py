#!/usr/bin/env python3
"""Timing of the device histograms of a saved trace (smcmc_trace_ranges, smcmc_marginal_histograms) beside existing code
that reads the same bytes in the same process: the autocorrelation reducer (smcmc_autocorrelation_sums: two passes over
the trace and a reduction; rocprofv3 --kernel-trace --stats over this command separates its kernels).

The trace is the largest of (512, 128, 32) slots x D = 50 x 65 536 chains that the card's free memory allows, written by
StepSave; every pass is timed on it and then on a trace of the same shape with every value identical (every count into
one bin: the contention worst case).  Each number is the time of the whole C call between two device events after one
warm-up call (it includes the call's own allocations and copies of a few KB to 2 MB), the least and the mean of --reps.
  bytes read: ranges  8 x sampled slots x dim x chains;  1-D fill  8 x slots x dim x chains;
              pair fill  8 x slots x chains x P (P + 1) / 2 rows (row i of the tables reads the dimensions i .. P - 1;
              the second read of dimension i itself hits the cache and is not counted);
              autocorrelation  8 x slots x dim x chains for each of its two passes (the second also reads the lagged block,
              mostly out of L2: not counted).
usage: python tools/marginals_time.py [--copies 16 4 64] [--reps 5] [--json profiles/marginals_time.json]
--copies: the number of private copies of the 1-D histogram per workgroup (SMCMC_MARGINAL_COPIES, read at every call)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--slots", type=int, nargs="+", default=[512, 128, 32], help="candidates, the largest that fits is used")
    ap.add_argument("--pair-dims", type=int, default=10)
    ap.add_argument("--copies", type=int, nargs="+", default=[16], help="1-D histogram copies to time (the first is the build's default)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "marginals_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    M = pkg.Marginals
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
    P = min(a.pair_dims, a.dim)
    dims = np.arange(P)
    rows = []

    def timed(name, nbytes, call, trace_kind, **extra):
        call()                                           # warm-up: code object, allocator
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        row = dict(pass_=name, trace=trace_kind, slots=slots, dim=a.dim, chains=a.chains, bytes_read=nbytes,
                   ms_min=min(ms), ms_mean=float(np.mean(ms)), TBps_at_min=nbytes / (min(ms) * 1e-3) / 1e12,
                   ps_per_byte_at_min=min(ms) * 1e9 / nbytes, **extra)
        row["pass"] = row.pop("pass_")
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    ptr, st = sx.data_ptr(), stream.cuda_stream
    macro_stride = M.macro_sample_stride(slots)
    for kind in ("engine", "identical"):
        if kind == "identical":
            sx.fill_(1.25)
            torch.cuda.synchronize()
            lo, hi = np.zeros(a.dim), np.full(a.dim, 2.0)                # every value in one bin of every axis
        else:
            m = e.Marginals(ptr, slots, stream=st)
            lo, hi = m.lo, m.hi
            assert np.all(m.counts1.sum(axis=1) == slots * a.chains)
        timed("autocorrelation (both passes + reduction)", 2 * value_bytes,
              lambda: e.AutocorrelationSums(ptr, slots, stream=st), kind)
        for stride in sorted({1, macro_stride}):
            sampled = len(range(0, slots, stride))
            timed("ranges", 8.0 * sampled * a.dim * a.chains,
                  lambda: e._lib.smcmc_trace_ranges(C.c_void_p(ptr), slots, a.dim, e.dim_padded, a.chains, e.nchains_padded, stride,
                                                    lo_out.ctypes.data_as(DP), hi_out.ctypes.data_as(DP), C.c_void_p(st)),
                  kind, sample_stride=stride)
        for copies in a.copies:
            os.environ["SMCMC_MARGINAL_COPIES"] = str(copies)
            timed("1-D fill, 100 bins", value_bytes,
                  lambda: e.Marginals(ptr, slots, n1=100, pair_dims=[], ranges=(lo, hi), stream=st), kind, copies=copies)
        os.environ.pop("SMCMC_MARGINAL_COPIES", None)
        timed("pair fill, P = %d, 50 x 50 bins" % P, 8.0 * slots * a.chains * P * (P + 1) / 2,
              lambda: e.Marginals(ptr, slots, n1=0, n2=50, pair_dims=dims, ranges=(lo, hi), stream=st), kind)
    floor_TBps = 8.0
    out = dict(device=torch.cuda.get_device_name(0), hbm_peak_TBps=floor_TBps, trace_bytes=float(slots * per_slot), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    e.close()


DP = C.POINTER(C.c_double)
lo_out, hi_out = np.zeros(4096), np.zeros(4096)

if __name__ == "__main__":
    main()
