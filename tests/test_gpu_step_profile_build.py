"""The profiling build of the step kernel (-DSMCMC_STEP_PROFILE, tools/micro/build_stepprof.sh: s_memtime stamps at the
section boundaries of the step loop) runs the same chains as the shipped library: a small pooled ensemble at D = 50, two
windows, identical accepted points, log-likelihoods, lanes and moments -- with the stamp buffer attached, and the
buffer filled.  Skipped when the profiling library has not been built (it is a development aid, not part of build())."""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF_DIR = os.path.join(ROOT, "root-simple-mcmc_amd", "build", "prof")
HEADER = open(os.path.join(ROOT, "root-simple-mcmc_amd", "csrc", "smcmc_kernels.hip.h")).read()
SLOTS = int(re.search(r"constexpr int kProfSlots = (\d+);", HEADER).group(1))                   # register pairs of sums per lane
SECTIONS = re.search(r"enum \{ (PROF_LOOP,.*?), PROF_COUNT \};", HEADER, re.S).group(1).count(",") + 1  # = PROF_COUNT
F64 = ("logl", "sigma", "acceptance", "acceptance_trials", "rigidity", "last_value", "last_x0", "step_rms", "logl_proposed")
I32 = ("trials", "successes", "next_update", "naccept", "step_rms_trials", "last_accept")


def _run(gpu, library, profile):
    import torch
    dim, chains, window = 50, 320, 256
    e = gpu.Engine(dim, chains, mode=gpu.MODE_POOLED, library=library)
    buf = None
    if profile:
        buf = torch.zeros(e.nchains_padded // 64 * SLOTS * 64, dtype=torch.int64, device="cuda")
        assert e._lib.smcmc_set_step_profile(e._h, ctypes.c_void_p(buf.data_ptr())) == 0
    assert e.Start(np.zeros(dim))
    e.Step(window)
    e.sync()
    e.Step(window)
    out = {"x": e.GetAccepted(), "covariance": e.covariance, "decomposition": e.decomposition}
    for name in F64 + I32:
        out[name] = e.lane(name)
    e.reduce_moments()
    out["moments"] = e.read_moments()
    torch.cuda.synchronize()
    cycles = buf.cpu().numpy() if profile else None
    e.close()
    return out, cycles


@pytest.mark.parametrize("level", [1, 2])
def test_stamped_kernel_runs_the_same_chains(gpu, level):
    lib = os.path.join(PROF_DIR, "libsmcmc_amd_stepprof%d.so" % level)
    if not os.path.exists(lib):
        pytest.skip("the profiling library is not built (tools/micro/build_stepprof.sh)")
    plain, _ = _run(gpu, None, False)
    stamped, cycles = _run(gpu, lib, True)
    for k in plain:
        assert np.array_equal(plain[k], stamped[k], equal_nan=True), f"level {level}: {k} differs"
    assert 0 < plain["naccept"].sum() < 512 * 320
    cycles = cycles.reshape(-1, SLOTS, 64)
    assert (cycles[:, 0, :SECTIONS] > 0).all()                       # every section of every wavefront was stamped
    assert (cycles[:, 1:, :].sum() > 0) == (level == 2)        # the per-piece slots only at level 2
