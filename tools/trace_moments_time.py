#!/usr/bin/env python3
"""Timing of the device mean / covariance sums of a saved trace (smcmc_trace_moments) and of the device Cholesky chain
(smcmc_cholesky_chain) beside existing code that reads the same bytes in the same process: the autocorrelation reducer
(smcmc_autocorrelation_sums: two passes over the trace and a reduction; rocprofv3 --kernel-trace --stats over this
command separates autocorr_partial_kernel<0>, its first pass, from the rest).

The trace is the largest of (512, 128, 32) slots x D = 50 x 65 536 chains that the card's free memory allows, written by
StepSave.  Each number is the time of the whole C call between two device events after one warm-up call (it includes
the call's own allocations and copies of a few KB to 5 MB), the least and the mean of --reps.
  bytes read:    moments  8 x slots x dim x chains;  autocorrelation  the same for each of its two passes
  bytes written: Cholesky fill  8 x slots x dim x chains (the store floor: those bytes at the HBM peak)
  matrix floor of the moments: tiles of the lower triangle of (dim + 1)^2 x 2 048 flops per 4 points at 78.6 TFLOP/s
usage: python tools/trace_moments_time.py [--reps 5] [--json profiles/trace_moments_time.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS = 8.0
FP64_MATRIX_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--slots", type=int, nargs="+", default=[512, 128, 32], help="candidates, the largest that fits is used")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "trace_moments_time.json"))
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
    tiles = (a.dim + 1 + 15) // 16
    matrix_floor_ms = tiles * (tiles + 1) / 2 * 2048.0 * slots * a.chains / 4 / (FP64_MATRIX_TFLOPS * 1e12) * 1e3
    hbm_floor_ms = value_bytes / (HBM_PEAK_TBPS * 1e12) * 1e3
    rows = []

    def timed(name, nbytes, call, **extra):
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
        row = {"pass": name, "slots": slots, "dim": a.dim, "chains": a.chains, "bytes": nbytes, "ms_min": min(ms),
               "ms_mean": float(np.mean(ms)), "TBps_at_min": nbytes / (min(ms) * 1e-3) / 1e12}
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    ptr, st = sx.data_ptr(), stream.cuda_stream
    centre = e.GetEstimatedCenter()
    m = e.TraceMoments(ptr, slots, centre=centre, stream=st)
    timed("trace moments", value_bytes, lambda: e.TraceMoments(ptr, slots, centre=centre, stream=st),
          hbm_floor_ms=hbm_floor_ms, matrix_floor_ms=matrix_floor_ms)
    timed("autocorrelation (both passes + reduction)", 2 * value_bytes,
          lambda: e.AutocorrelationSums(ptr, slots, centre=centre, stream=st), hbm_floor_ms=2 * hbm_floor_ms)
    # the stand-in chain of what the trace holds, filled into the same buffer: the same shape, 13.4 GB written
    import ctypes as C
    mean, cov = np.ascontiguousarray(m.mean), np.ascontiguousarray(m.covariance)
    DP = C.POINTER(C.c_double)

    def fill():
        status = e._lib.smcmc_cholesky_chain(mean.ctypes.data_as(DP), cov.ctypes.data_as(DP), a.dim, slots, a.chains,
                                             e.nchains_padded, e.dim_padded, 20240607, 0, C.c_void_p(ptr), None, C.c_void_p(st))
        assert status == 0, status
    timed("cholesky chain fill", value_bytes, fill, hbm_floor_ms=hbm_floor_ms)
    g = e.TraceMoments(ptr, slots, centre=mean, stream=st)    # the round trip, as a sanity check of what was timed
    n = float(slots) * a.chains
    worst = float(np.max(np.abs(g.mean - mean) / np.sqrt(np.diag(cov) / n)))
    print("round trip: worst |mean - input| = %.2f standard errors" % worst, flush=True)
    out = dict(device=torch.cuda.get_device_name(0), hbm_peak_TBps=HBM_PEAK_TBPS, fp64_matrix_TFLOPS=FP64_MATRIX_TFLOPS,
               trace_bytes=float(slots * per_slot), round_trip_worst_mean_sigmas=worst, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    e.close()


if __name__ == "__main__":
    main()
