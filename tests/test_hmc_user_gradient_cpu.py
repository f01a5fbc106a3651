"""HMC with the caller's own gradient, the host side: the Python restatement of one fixed-step TSimpleHMC::Step
(tests/hmc_gradient_ref.py) against oracle.Hmc, the example library of a user likelihood with a gradient
(examples/user_likelihood_quadgrad.hip.h), the ABI additions and the BadGrad driver's compile.  All of it runs without a
GPU except test_which_engines_have_a_gradient, which is marked gpu: smcmc_hmc_has_gradient takes an engine, and an
engine needs a device to exist (without one the symbol's presence and its NULL answer are what can be checked)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from hmc_gradient_ref import HmcGradientRef  # noqa: E402
from hmc_user_gradient_cases import ASYM_HEADER, ASYM_LIB, GRAD_LIB, grad_lib, spd_matrix  # noqa: E402

@pytest.mark.parametrize("from_gradient", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("dim", [3, 8])
def test_restatement_is_the_oracle_chain_when_the_gradient_is_the_likelihoods_own(oracle, dim, alpha, from_gradient):
    err = spd_matrix(dim, 100 + dim)
    eps, L, steps, seed, cid = 0.12, 4, 10, 77, 3
    ora = oracle.Hmc(dim, kind=oracle.LIKE_QUADFORM, params=err, seed=seed, chain_id=cid,
                     potential_from_gradient=from_gradient)
    ref = HmcGradientRef(oracle, dim,
                         gradient=lambda q: oracle.hmc_gradient(oracle.LIKE_QUADFORM, q, params=err),
                         potential=lambda q: oracle.hmc_potential(oracle.LIKE_QUADFORM, q, params=err,
                                                                  potential_from_gradient=from_gradient),
                         abs_epsilon=eps, leapfrog=L, alpha=alpha, seed=seed, chain_id=cid)
    x0 = np.random.default_rng(dim).uniform(-1.0, 1.0, dim)
    ora.start(x0)
    ora.set_alpha(alpha); ora.set_mean_epsilon(-eps); ora.set_leapfrog(L)
    ref.start(x0)
    naccept = 0
    for s in range(steps):
        ora.step()
        ref.step()
        sc = ora.scalars
        naccept += int(sc["last_accept"])
        assert np.array_equal(ora.accepted, np.array(ref.accepted)), f"step {s}"
        assert np.array_equal(ora.momentum, np.array(ref.momentum)), f"step {s}"
        assert sc["accepted_potential"] == ref.accepted_potential and sc["proposed_potential"] == ref.proposed_potential
        assert sc["current_acceptance"] == ref.acceptance
        assert naccept == ref.naccept
    assert 0 < naccept


def test_gradient_library_builds_and_exports_the_whole_c_abi(smcmc):
    lib = smcmc.load(grad_lib(smcmc))
    for name in smcmc.SIGNATURES:
        assert hasattr(lib, name)
    assert "smcmc_hmc_has_gradient" in smcmc.SIGNATURES and "smcmc_hmc_set_gradient_matrix" in smcmc.SIGNATURES


def test_two_user_libraries_live_side_by_side(smcmc):
    """--output-name: the asym example and the gradient example are two files made from two sets of user objects."""
    grad_lib(smcmc)
    if not os.path.exists(ASYM_LIB):
        smcmc._build_mod.build(user_likelihood=ASYM_HEADER)
    assert os.path.exists(ASYM_LIB) and os.path.exists(GRAD_LIB)
    obj = os.path.join(ROOT, "root-simple-mcmc_amd", "build")
    assert os.path.exists(os.path.join(obj, "hmc_engine_user.o")) and os.path.exists(os.path.join(obj, "hmc_engine_user_grad.o"))


def _has_gradient(lib, like, dim=4):
    h = C.c_void_p()
    st = lib.smcmc_hmc_create(dim, 8, like, 1, 0, 0, C.byref(h))
    if st != 0:
        return st, None
    try:
        return st, lib.smcmc_hmc_has_gradient(h)
    finally:
        lib.smcmc_hmc_destroy(h)


def test_has_gradient_is_null_safe(smcmc):
    assert smcmc.load().smcmc_hmc_has_gradient(None) == 0
    assert smcmc.load().smcmc_hmc_set_gradient_matrix(None, None, 0) == 1    # SMCMC_ERR_INVALID


@pytest.mark.gpu
def test_which_engines_have_a_gradient(gpu):
    """smcmc_hmc_has_gradient: 1 for ISO / QUADFORM / ROSENBROCK and a user library with a gradient, 0 otherwise (an engine
    needs a device to exist, so this one is a GPU test)."""
    plain = gpu.load()
    for like, want in ((gpu.LIKE_ISO_GAUSS, 1), (gpu.LIKE_QUADFORM, 1), (gpu.LIKE_ROSENBROCK, 1), (gpu.LIKE_ASYM, 0),
                       (gpu.LIKE_HORRIFIC, 0), (gpu.LIKE_CONSTRAINED, 0)):
        assert _has_gradient(plain, like) == (0, want), like
    assert _has_gradient(gpu.load(grad_lib(gpu)), gpu.LIKE_USER) == (0, 1)
    if not os.path.exists(ASYM_LIB):
        gpu._build_mod.build(user_likelihood=ASYM_HEADER)
    assert _has_gradient(gpu.load(ASYM_LIB), gpu.LIKE_USER) == (0, 0)
    assert gpu.HmcEngine(4, 8, likelihood=gpu.LIKE_ISO_GAUSS).has_gradient is True


def test_a_gradient_without_the_any_dimension_form_is_refused_at_compile_time(tmp_path):
    hdr = tmp_path / "bad_user.hip.h"
    hdr.write_text("#pragma once\n"
                   "template <int DP> __device__ double smcmc_user_loglike(const double (&p)[DP], smcmc::cptr_f64, int) { return -p[0] * p[0]; }\n"
                   "#define SMCMC_USER_GRADIENT 1\n"
                   "template <class Point> __device__ double smcmc_user_gradient_at(const Point& p, const double*, int, int i) { return -2.0 * p[i]; }\n")
    csrc = os.path.join(ROOT, "root-simple-mcmc_amd", "csrc")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only",
                        f"-I{os.path.join(ROOT, 'include')}", f"-I{csrc}", f'-DSMCMC_USER_LIKELIHOOD="{hdr}"',
                        os.path.join(csrc, "smcmc_hmc_engine.hip")], capture_output=True, text=True)
    assert r.returncode != 0
    assert "SMCMC_USER_GRADIENT needs SMCMC_USER_LIKELIHOOD_ANY_DIM" in r.stderr


def test_badgrad_driver_compiles(tmp_path):
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}", "-c",
                        os.path.join(ROOT, "examples", "BadGrad_amd.C"), "-o", str(tmp_path / "badgrad.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
