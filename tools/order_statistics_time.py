#!/usr/bin/env python3
"""Timing of the exact quantiles of a saved trace (smcmc_trace_order_statistics through Quantiles / PredictiveQuantiles
with the five default probabilities: ten ranks, or fewer where two coincide) beside two yardsticks taken in the same
process on the same card, recorded in profiles/order_statistics_notes.md:
  * eight plain reads of the rows' bytes at --read-tbps, the rate profiles/marginals_notes.md records for a kernel that
    only reads a trace (trace_ranges_partial_kernel, 6.1 TB/s): the floor of an eight-pass selection;
  * torch.sort along the flattened (slot, chain) axis of the same rows: the off-the-shelf alternative, timed without and
    with the copy that lays the rows out for it.
Sizes: D = 50 x 65 536 chains x 16 slots and D = 9 x 16 384 chains x 16 slots, saved by StepSave from a pooled ensemble,
and the predictive buffer of example/'s sample (150 rows x 16 384 chains x 16 slots) as PosteriorPredictive fills it.
Each figure: --warmup calls first, then the least and the median of --reps calls between two device events; the reducer's
figure is the whole C call (its allocation, its 17 launches, the copy of the results back).
usage: python tools/order_statistics_time.py [--reps 5] [--json profiles/order_statistics_time.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from event_sample_time import timed, toy_sample  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--read-tbps", type=float, default=6.1)
    ap.add_argument("--cases", nargs="+", default=["50x65536", "9x16384", "predictive"])
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "order_statistics_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    rows = []

    def measure(name, quantiles, buf, nrows, nchains, nslots):
        """quantiles(): the reducer's call; buf[slot][stride][npad]: what it reads"""
        nbytes = 8.0 * nslots * nrows * nchains
        tq = quantiles()
        lo, med = timed(torch, stream, quantiles, a.warmup, a.reps)

        def gather():
            return buf[:, :nrows, :nchains].permute(1, 0, 2).reshape(nrows, -1)
        flat = gather()
        s_lo, s_med = timed(torch, stream, lambda: torch.sort(flat, dim=1), a.warmup, a.reps)
        g_lo, g_med = timed(torch, stream, lambda: torch.sort(gather(), dim=1), a.warmup, a.reps)
        # what was timed is what the sort gives
        ordered = torch.sort(flat, dim=1).values
        agree = bool(torch.equal(ordered[:, tq.ranks.astype(np.int64)].cpu(), torch.from_numpy(tq.values)))
        rows.append(dict(case=name, rows=nrows, chains=nchains, slots=nslots, bytes=nbytes, ranks=int(tq.ranks.size),
                         quantiles_ms_min=lo, quantiles_ms_median=med, eight_reads_floor_ms=8 * nbytes / (a.read_tbps * 1e12) * 1e3,
                         TBps_over_eight_reads=8 * nbytes / (lo * 1e-3) / 1e12, torch_sort_ms_min=s_lo, torch_sort_ms_median=s_med,
                         torch_gather_and_sort_ms_min=g_lo, torch_gather_and_sort_ms_median=g_med, equals_torch_sort=agree))
        print(json.dumps(rows[-1]), flush=True)
        del flat, ordered

    for case in a.cases:
        if case == "predictive":
            nchains = 16384
            params = toy_sample(pkg)
            e = pkg.Engine(9, nchains, likelihood=pkg.LIKE_EVENT_SAMPLE, likelihood_params=params, mode=pkg.MODE_POOLED, stream=st)
            assert e.Start(np.zeros(9))
            sx = torch.empty((a.slots, e.dim_padded, e.nchains_padded), dtype=torch.float64, device="cuda")
            sl = torch.empty((a.slots, e.nchains_padded), dtype=torch.float64, device="cuda")
            e.StepSave(a.slots, sx.data_ptr(), sl.data_ptr(), stride=1)
            nrows = 3 * int(params[1])
            hist = torch.empty((a.slots, nrows, e.nchains_padded), dtype=torch.float64, device="cuda")
            e.PosteriorPredictive(sx.data_ptr(), a.slots, histograms_ptr=hist.data_ptr(), stream=st)
            torch.cuda.synchronize()
            measure("predictive buffer of example/", lambda: e.PredictiveQuantiles(hist.data_ptr(), a.slots, stream=st), hist,
                    nrows, nchains, a.slots)
            del hist
        else:
            dim, nchains = (int(v) for v in case.split("x"))
            e = pkg.Engine(dim, nchains, mode=pkg.MODE_POOLED, stream=st)
            assert e.Start(np.zeros(dim))
            for _ in range(4):                               # the pooled proposal adapts: a realistic posterior sample
                e.Step(64)
                e.sync()
            sx = torch.empty((a.slots, e.dim_padded, e.nchains_padded), dtype=torch.float64, device="cuda")
            sl = torch.empty((a.slots, e.nchains_padded), dtype=torch.float64, device="cuda")
            e.StepSave(a.slots * 2, sx.data_ptr(), sl.data_ptr(), stride=2)
            torch.cuda.synchronize()
            measure("trace D = %d x %d chains" % (dim, nchains), lambda: e.Quantiles(sx.data_ptr(), a.slots, stream=st), sx, dim,
                    nchains, a.slots)
        del sx, sl
        e.close()
    out = dict(device=torch.cuda.get_device_name(0), read_TBps=a.read_tbps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
