#!/usr/bin/env python3
"""Timing of the posterior-predictive check (smcmc_predictive_check, Engine.PredictiveCheck) beside what it is an
accessory of, taken in the same process on the same card, recorded in profiles/predictive_check_notes.md:
  * SMCMC_LIKE_EVENT_SAMPLE at example/'s own size (tools/event_sample_time.py's sample: three histograms of 50 bins), a
    trace of --slots x --chains points saved by StepSave, as tools/event_predictive_time.py sets it up;
  * the PosteriorPredictive call that fills the buffer of every point's histograms, sums alone and with the histograms
    and the log-likelihood written (the yardstick, re-measured here);
  * the check over that buffer, the whole C call between two device events, without and with its two optional outputs
    (the replicates and the statistics of every point);
  * a device-to-device copy of the same buffer on the same stream: one read (and one write) of it, the floor;
  * the check over --cost-slots slots of that buffer with every mean at 1e4 and at 2^20: the O(sqrt(mu)) cost of the
    variate (fewer slots: at 2^20 a variate is some 800 terms and a wavefront waits for its slowest lane).
Each figure: --warmup calls first, then the least and the median of --reps calls.
usage: python tools/predictive_check_time.py [--reps 3] [--json profiles/predictive_check_time.json]"""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--cost-slots", type=int, default=1)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "predictive_check_time.json"))
    a = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    params = toy_sample(pkg)
    e = pkg.Engine(9, a.chains, likelihood=pkg.LIKE_EVENT_SAMPLE, likelihood_params=params, mode=pkg.MODE_POOLED, stream=st)
    assert e.Start(np.zeros(9))
    npad, stride = e.nchains_padded, e.dim_padded
    sx = torch.empty((a.slots, stride, npad), dtype=torch.float64, device="cuda")
    sl = torch.empty((a.slots, npad), dtype=torch.float64, device="cuda")
    e.StepSave(a.slots, sx.data_ptr(), sl.data_ptr(), stride=1)
    torch.cuda.synchronize()
    points = a.slots * a.chains
    base = {"likelihood": "SMCMC_LIKE_EVENT_SAMPLE", "nevents": int(params[0]), "nbins": int(params[1]), "slots": a.slots,
            "chains": a.chains}
    rows = []

    def record(case, lo, med, **more):
        rows.append(dict(base, case=case, ms_min=lo, ms_median=med, points_per_s=points / (lo * 1e-3), **more))
        print(json.dumps(rows[-1]), flush=True)

    ptr = sx.data_ptr()
    first = e.PosteriorPredictive(ptr, a.slots, stream=st)
    centre = np.where(np.isfinite(first.mean), first.mean, 0.0)
    nrows = first.data.size
    hist = torch.empty((a.slots, nrows, npad), dtype=torch.float64, device="cuda")
    logl = torch.empty((a.slots, npad), dtype=torch.float64, device="cuda")
    record("posterior predictive, sums alone",
           *timed(torch, stream, lambda: e.PosteriorPredictive(ptr, a.slots, centre=centre, stream=st), a.warmup, a.reps))
    record("posterior predictive, histograms and logl of every point written",
           *timed(torch, stream, lambda: e.PosteriorPredictive(ptr, a.slots, centre=centre, histograms_ptr=hist.data_ptr(),
                                                               logl_ptr=logl.data_ptr(), stream=st), a.warmup, a.reps))
    nbytes = 8.0 * a.slots * nrows * npad
    live = hist[:, :, :a.chains]
    record("predictive check, counts alone",
           *timed(torch, stream, lambda: e.PredictiveCheck(hist.data_ptr(), a.slots, stream=st), a.warmup, a.reps),
           bytes_read=nbytes, mean_of_means=float(live.mean()), largest_mean=float(live.max()))
    rep = torch.empty_like(hist)
    stat = torch.empty((a.slots, 2 * (first.data.shape[0] + 1), npad), dtype=torch.float64, device="cuda")
    record("predictive check, replicates and statistics of every point written",
           *timed(torch, stream, lambda: e.PredictiveCheck(hist.data_ptr(), a.slots, replicates_ptr=rep.data_ptr(),
                                                           statistics_ptr=stat.data_ptr(), stream=st), a.warmup, a.reps),
           bytes_read=nbytes, bytes_written=nbytes + 8.0 * stat.numel())
    pc = e.PredictiveCheck(hist.data_ptr(), a.slots, stream=st)
    print(json.dumps({"pvalue": pc.pvalue, "group_pvalues": pc.group_pvalues, "n": pc.n, "invalid": pc.invalid}), flush=True)
    record("device-to-device copy of the buffer (the floor)", *timed(torch, stream, lambda: rep.copy_(hist), a.warmup, a.reps),
           bytes_read=nbytes, bytes_written=nbytes)
    points = a.cost_slots * a.chains
    for mean in (1.0e4, 2.0 ** 20):
        hist[:a.cost_slots].fill_(mean)
        torch.cuda.synchronize()
        record("predictive check, counts alone, every mean %g" % mean,
               *timed(torch, stream, lambda: e.PredictiveCheck(hist.data_ptr(), a.cost_slots, stream=st), a.warmup, a.reps),
               slots_timed=a.cost_slots, bytes_read=nbytes * a.cost_slots / a.slots)
    e.close()
    out = dict(device=torch.cuda.get_device_name(0), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
