"""Per-step time of the HMC engine's SMCMC_MODE_PER_CHAIN against SMCMC_MODE_POOLED with a sync every step, default
tuning (SimpleHMC.C's call sequence), timed after 2 D warm-up steps, on the GPU box:

    python tools/hmc_perchain_time.py [--steps K] [--shapes iso50x64,iso50x4096,iso50x16384,quad200x1024]

For the per-chain mode it also prints the model of the kernels that mode adds after every step (hmc_pc_exxt_kernel and
hmc_pc_decide_kernel): the bytes they move at 8 TB/s against the FP64 issue of their divides, whichever is larger.  The
error-matrix kernel runs only for the chains whose update goes through; its share shows in a kernel trace."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
FP64_LANE_OPS_PER_S = 256 * 64 * 2.4e9      # 256 CUs x 64 FP64 lanes per clock x 2.4 GHz
DIVIDE_OPS = 10                             # v_div_scale x2, v_rcp, 4 x v_fma, v_mul, v_div_fmas, v_div_fixup


def model(dim, nchains):
    npk = dim * (dim + 1) // 2
    words = (2 * npk                        # fEXXT read + write
             + dim                          # the pre-step point (once per chain; the rest of its reads hit the caches)
             + 3 * dim                      # fAveragePoint read + write, the pre-step point again
             + dim                          # the diagonal of fEXXT for the trace
             + 2 * 12)                      # tuning scalars and lanes
    nbytes = 8.0 * words * nchains
    divides = (npk + dim) * nchains
    t_bytes = nbytes / HBM_BYTES_PER_S
    t_div = divides * DIVIDE_OPS / FP64_LANE_OPS_PER_S
    return nbytes, divides, t_bytes, t_div, max(t_bytes, t_div)


def parse(shape):
    kind, rest = ("quad", shape[4:]) if shape.startswith("quad") else ("iso", shape[3:])
    d, n = rest.split("x")
    return kind, int(d), int(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shapes", default="iso50x64,iso50x4096,iso50x16384,quad200x1024")
    ap.add_argument("--modes", default="per_chain,pooled")
    args = ap.parse_args()
    import torch
    from smcmc_amd_loader import load_package
    pkg = load_package()
    stream = torch.cuda.current_stream().cuda_stream
    for shape in args.shapes.split(","):
        kind, dim, n = parse(shape)
        prm = None
        like = pkg.LIKE_ISO_GAUSS
        if kind == "quad":
            rng = np.random.default_rng(3)
            a = rng.standard_normal((dim, dim)) / np.sqrt(dim)
            prm = np.linalg.inv(a @ a.T + np.eye(dim))
            like = pkg.LIKE_QUADFORM
        for mode_name in args.modes.split(","):
            mode = pkg.MODE_PER_CHAIN if mode_name == "per_chain" else pkg.MODE_POOLED
            e = pkg.HmcEngine(dim, n, likelihood=like, likelihood_params=prm, seed=11, stream=stream, mode=mode)
            e.SetSyncInterval(1)
            e.Start(np.full(dim, 0.5))
            e.Step(2 * dim)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.Step(args.steps)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            out = {"shape": shape, "mode": mode_name, "dim": dim, "nchains": n, "steps": args.steps,
                   "step_ms": round(dt * 1e3, 4), "chain_steps_per_s": round(n / dt, 1),
                   "leapfrog_mean": float(np.mean(np.abs(e.lane("leapfrog"))))}
            if mode == pkg.MODE_PER_CHAIN:
                nbytes, divides, tb, td, tm = model(dim, n)
                tun = [e.chain_tuning(c)[2]["updates"] for c in range(0, n, max(1, n // 64))]
                out.update({"model_bytes": nbytes, "model_divides": divides, "model_bytes_us": round(tb * 1e6, 2),
                            "model_divides_us": round(td * 1e6, 2), "model_us": round(tm * 1e6, 2),
                            "updates_mean_sampled": float(np.mean(tun))})
            print(json.dumps(out), flush=True)
            e.close()


if __name__ == "__main__":
    main()
