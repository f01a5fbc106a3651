"""The statistical case of tests/test_gpu_hmc_user_gradient.py on the CPU, before the GPU test is relied on: the first
1 024 of its chains run through tests/hmc_gradient_ref.py (the Python restatement of the reference step) with the same
wrong gradient matrix, start points and random streams, and the same bounds computed with n = 1 024.

  python tools/hmc_bad_gradient_cpu_check.py [nchains]
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
from hmc_gradient_ref import HmcGradientRef  # noqa: E402
from hmc_user_gradient_cases import (STAT_DIM, STAT_EPS, STAT_LEAP, STAT_MAX_CURVATURE, STAT_SEED, STAT_STEPS, badgrad_matrices,  # noqa: E402
                                     stat_bounds_hold, stat_start_points)

O.build()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
cov, err, gerr = badgrad_matrices(STAT_DIM, STAT_SEED, STAT_MAX_CURVATURE)
print("eigenvalues of Error        ", np.round(np.linalg.eigvalsh(err), 3))
print("eigenvalues of GradientError", np.round(np.linalg.eigvalsh(gerr), 3))
x0 = stat_start_points(cov)[:, :n]
q = np.zeros((STAT_DIM, n))
naccept = 0
for c in range(n):
    r = HmcGradientRef(O, STAT_DIM,
                       gradient=lambda p: O.hmc_gradient(O.LIKE_QUADFORM, p, params=gerr),
                       potential=lambda p: O.hmc_potential(O.LIKE_QUADFORM, p, params=err, potential_from_gradient=True),
                       abs_epsilon=STAT_EPS, leapfrog=STAT_LEAP, seed=STAT_SEED, chain_id=c)
    r.start(x0[:, c])
    r.run(STAT_STEPS)
    q[:, c] = r.accepted
    naccept += r.naccept
print(f"{n} chains x {STAT_STEPS} steps: accepted {naccept} of {n * STAT_STEPS}")
ok = stat_bounds_hold(q, cov)
print("inside the bounds" if ok else "OUTSIDE the bounds")
sys.exit(0 if ok else 1)
