"""The C++ mirror and the user-likelihood build on the streamed one-chain-per-workgroup kernel
(SMCMC_P_PERCHAIN_STREAM): SetPerChainAdaptation(true) above smcmc_max_perchain_dim(), Step() one call at a time with
run-ahead on, and SMCMC_LIKE_USER."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_perchain_workgroup import _accepted, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USER_LIB = os.path.join(ROOT, "root-simple-mcmc_amd", "lib", "libsmcmc_amd_user.so")

pytestmark = pytest.mark.gpu


def test_step_per_call_runs_ahead_and_is_the_reference_chain(gpu, oracle, tmp_path):
    """One chain at D = 200 through TSimpleMCMC_amd.H with SetPerChainAdaptation(true): Step(true) per call, run-ahead
    off, on, and turned off after the first cycle.  Every tree is the same, and its Accepted column is oracle.Chain's
    under the driver's settings."""
    exe = _build(tmp_path)
    dim, cycles, steps = 200, 2, 150
    trees = []
    for ahead in (0, 1, 2):
        out = tmp_path / f"tree{ahead}.csv"
        r = subprocess.run([exe, str(dim), str(cycles), str(steps), "1", str(ahead), str(out), "1"],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"run_ahead {1 if ahead == 1 else 0}" in r.stdout
        trees.append(open(out).read())
    assert trees[0] == trees[1] == trees[2]
    got = _accepted(tmp_path / "tree1.csv", dim)
    assert len(got) == cycles * steps + 1

    c = oracle.Chain(dim, chain_id=0)
    assert c.start(np.zeros(dim))
    c.set_acceptance_window(1000)                                 # the driver's settings (SimpleMCMC.C:196-200)
    c.set_acceptance_rigidity(2.0)
    c.set_covariance_window(cycles * steps)
    c.set_covariance_deweight(0.20)
    c.set_next_update(1E+9)
    row = 0
    for _ in range(cycles):
        for _ in range(steps):
            c.step(True, 0)
            assert np.array_equal(got[row], c.accepted), f"entry {row}"
            row += 1
        c.update_proposal()
        c.set_acceptance_rigidity(2.0)
        c.set_covariance_deweight(0.0)
        c.set_next_update(10 * steps)
    assert np.array_equal(got[row], c.accepted)                   # the final SaveStep()


def test_user_likelihood_on_the_streamed_kernel(gpu, oracle):
    """The user build's SMCMC_LIKE_USER instantiation (examples/user_likelihood_asym.hip.h, the reference's
    TAsymLogLikelihood) at D = 157 is oracle.Chain(kind=ASYM), bit for bit."""
    assert os.path.exists(USER_LIB), "__graft_entry__.build() makes it"
    dim, n = 157, 3
    prm = np.array([-1.0, 100.0])
    e = gpu.Engine(dim, n, likelihood=gpu.LIKE_USER, likelihood_params=prm, mode=gpu.MODE_PER_CHAIN,
                   perchain_stream=True, library=USER_LIB)
    assert e.get_param("PERCHAIN_STREAM") == 1
    chains = {c: oracle.Chain(dim, kind=oracle.LIKE_ASYM, params=prm, chain_id=c) for c in range(n)}
    x0 = np.random.default_rng(dim + 28).uniform(0.5, 1.5, size=(dim, n))   # (off the peak: moves are accepted)
    assert e.Start(x0)
    for c, ch in chains.items():
        assert ch.start(x0[:, c])
    for _ in range(3):                                            # UpdateProposal inside the launches
        e.SetNextUpdate(12)
        e.Step(300)
        for ch in chains.values():
            ch.set_next_update(12)
            ch.run_quiet(300)
    x = e.GetAccepted()
    for c, ch in chains.items():
        assert np.array_equal(x[:, c], ch.accepted), f"chain {c}"
        centre, cov, dec = e.chain_proposal(c)
        assert np.array_equal(cov, ch.covariance) and np.array_equal(dec, ch.decomposition), f"chain {c}"
        assert e.lane("logl")[c] == ch.scalars["accepted_logl"]
    assert np.all(e.lane("update_count") >= 2)
