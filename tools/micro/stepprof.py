"""Section profile of the headline step kernel (GPU box): cycles per wavefront-step by section of the step loop, from the
s_memtime stamps of the profiling build (tools/micro/build_stepprof.sh, SMCMC_STEP_PROFILE in smcmc_kernels.hip.h).
Level 1 stamps the sections only, level 2 every piece too.  A stamp waits for its own value and drains the LDS queue, so
each figure is printed raw and with the stamps' own cost (section "stamp": two stamps back to back) taken off.  The
compiler sinks the additions into the per-section sums to the end of the loop body: section "loop back + profile sums" is
mostly the profile's own arithmetic (it grows with the number of stamps) and is not part of the plain kernel's step.
usage: python tools/micro/stepprof.py [level [windows [pooled|frozen]]]"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from smcmc_amd_loader import load_package  # noqa: E402
import torch  # noqa: E402

pkg = load_package()
level = int(sys.argv[1]) if len(sys.argv) > 1 else 1
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 4
mode = sys.argv[3] if len(sys.argv) > 3 else "pooled"
lib = os.path.join(ROOT, "root-simple-mcmc_amd", "build", "prof", "libsmcmc_amd_stepprof%d.so" % level)
dim, chains, steps = 50, 65536, 256
SECTIONS = ["loop back + profile sums", "stamp", "a scalar half of UpdateState", "b top of step", "c normals (13 blocks)", "d pieces, rest",
            "tail of the proposal", "e step-RMS sum", "e likelihood", "e accept test", "e commit writes", "e end-of-step wait"]
STAMPS = [1, 1, 1, 1, 13, 13, 1, 1, 1, 1, 1, 1]      # stamps per step that end in each section
KINDS = ["read drain", "vector arithmetic", "matrix part"]

pooled = mode == "pooled"
e = pkg.Engine(dim, chains, mode=pkg.MODE_POOLED if pooled else pkg.MODE_FROZEN, library=lib)
assert e.Start(np.zeros(dim))
for _ in range(3):
    e.Step(steps)
    if pooled:
        e.sync()
groups = e.nchains_padded // 64
buf = torch.zeros(groups * 7 * 64, dtype=torch.int64, device="cuda")
assert e._lib.smcmc_set_step_profile(e._h, ctypes.c_void_p(buf.data_ptr())) == 0
for _ in range(windows):
    e.Step(steps)
    if pooled:
        e.sync()
torch.cuda.synchronize()
assert e._lib.smcmc_set_step_profile(e._h, None) == 0
c = buf.cpu().numpy().reshape(groups, 7, 64).astype(np.float64).mean(axis=0) / (windows * steps)
e.close()

cost = c[0, 1]
print("D = %d, %d chains, %s, level %d, %d windows of %d steps: cycles per wavefront-step (mean over %d wavefronts)"
      % (dim, chains, mode, level, windows, steps, groups))
print("%-32s %10s %8s %10s" % ("section", "raw", "stamps", "net"))
total_raw = total_net = 0.0
for k, name in enumerate(SECTIONS):
    net = c[0, k] - STAMPS[k] * cost
    total_raw += c[0, k]
    total_net += net
    print("%-32s %10.0f %8d %10.0f" % (name, c[0, k], STAMPS[k], net))
if level >= 2:
    pieces = c[1:].reshape(3, 128)
    npieces = int((pieces[1] > 0).sum())
    for q, kind in enumerate(KINDS):
        raw = pieces[q, :npieces].sum()
        net = raw - npieces * cost
        total_raw += raw
        total_net += net
        print("%-32s %10.0f %8d %10.0f" % ("d pieces, " + kind, raw, npieces, net))
print("%-32s %10.0f %8s %10.0f   (one stamp: %.0f)" % ("total", total_raw, "", total_net, cost))
if level >= 2:
    net = pieces[:, :npieces] - cost
    worst = np.argsort(-net[0])[:3]
    print("worst three pieces by read drain (net): " + ", ".join("piece %d: %.0f" % (g, net[0, g]) for g in worst))
    print("piece: read drain / vector arithmetic / matrix part (net of one stamp each)")
    for g in range(npieces):
        print("  %3d %6.0f %6.0f %6.0f" % (g, net[0, g], net[1, g], net[2, g]))
