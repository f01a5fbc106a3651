"""Every device path that decomposes a covariance, judged by the verdicts of tests/linalg_truth.py against an independent
truth rather than against the host or the oracle: the pooled update's two Cholesky kernels (one workgroup; 32-row
panels), the host ladder behind them, the three per-chain kernels, smcmc_cholesky_chain's factor, and the per-chain HMC
mode's Householder + QL routine.  The matrix judged against is always the covariance the engine hands back, i.e. the one
the decomposition read; where nothing can have touched it, it must also be the injected matrix bit for bit.

The constants (tests/linalg_truth.py): eigen rung K = 450 = 100 x 4.50, QL K = 53.76 = 32 x 1.68, each factor times the
worst figure numpy's LAPACK shows on the same matrices against the same truth."""
import importlib.util
import os
import sys

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("smcmc_linalg_truth", os.path.join(os.path.dirname(os.path.abspath(__file__)), "linalg_truth.py"))
T = sys.modules.get("smcmc_linalg_truth") or importlib.util.module_from_spec(_spec)
if "smcmc_linalg_truth" not in sys.modules:
    sys.modules["smcmc_linalg_truth"] = T
    _spec.loader.exec_module(T)

pytestmark = pytest.mark.gpu

NCHAINS = 64
_CASES = {}


def cases(n):
    """Families (a)-(g) at size n, built once per module: truths are cached on the cases."""
    if n not in _CASES:
        extra = T.decision_pair(n, 1e-10, graded_by=0) if n > T.SOLVE_LIMIT else []
        _CASES[n] = T.cholesky_cases(n) + extra
    return _CASES[n]


def nan_case(n):
    return T.non_finite(n)[0]


# ---- pooled ------------------------------------------------------------------------------------------------------------

def _pooled(gpu, n, device_update, A):
    e = gpu.Engine(n, NCHAINS, mode=gpu.MODE_POOLED)
    e.set_param("DEVICE_UPDATE", device_update)
    assert e.Start(np.zeros(n))
    e.Step(1)
    e.sync()
    e.SetCovariance(A)
    e.set_param("COVARIANCE_TRIALS", 1e30)               # the folded points move no term by more than a rounding
    updates = e.get_param("UPDATE_COUNT")
    e.Step(1)
    e.sync()
    assert e.get_param("UPDATE_COUNT") == updates + 1
    out = int(e.get_param("LAST_UPDATE_PATH")), e.covariance, e.decomposition
    e.close()
    return out


@pytest.mark.parametrize("device_update", [1, 0])
@pytest.mark.parametrize("n", [2, 33, 63, 64, 65, 96, 129])
def test_pooled_update(gpu, n, device_update):
    """SetCovariance, COVARIANCE_TRIALS = 1e30, Step, sync: the pooled update decomposes the running covariance, which is
    the injected one to a rounding (v T + b) / (T + n).  n <= 64 is the one-workgroup kernel, above it the 32-row
    panels (65: a panel of one row; 96: three full panels; 129: four and one row); a matrix the device refuses goes down
    the host ladder.  DEVICE_UPDATE = 0 is the all-host update; with 1 the engine takes the device kernels whenever the
    mode is pooled and no dimension is uniform (device_update_eligible in smcmc_engine.hip), which holds here, and no
    call reports which one ran.  Both pass the same verdicts: Cholesky residual within
    gamma_(n+1) |U^T||U| on paths 0, 1 and 3, eigen rung with K = 450 on path 2, the decision by Higham Thm 10.7."""
    for case in cases(n):
        path, cov, dec = _pooled(gpu, n, device_update, case.A)
        tag = f"{case} DEVICE_UPDATE={device_update}"
        assert T._fro(cov - case.A) <= 4 * T.U * T._fro(case.A) or path >= 1, tag
        T.check_ladder(case, path, path == 2, cov, dec, tag, injected=False)
    path, cov, dec = _pooled(gpu, n, device_update, nan_case(n))
    assert path >= 1 and np.all(np.isfinite(dec))


# ---- frozen ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 33, 65])
def test_frozen_update_proposal(gpu, n):
    """MODE_FROZEN: SetCovariance, UpdateProposal.  Nothing folds, so on path 0 the covariance read back is the injected
    matrix bit for bit.  The families reach paths 0, 1 and 2."""
    seen = set()
    for case in cases(n) + [T.over_correlated(n)]:
        e = gpu.Engine(n, NCHAINS, mode=gpu.MODE_FROZEN)
        assert e.Start(np.zeros(n))
        e.SetCovariance(case.A)
        e.UpdateProposal()
        path = int(e.get_param("LAST_UPDATE_PATH"))
        T.check_ladder(case, path, path == 2, e.covariance, e.decomposition, f"frozen {case}")
        seen.add(path)
        e.close()
    assert {0, 1, 2} <= seen


# ---- per chain -----------------------------------------------------------------------------------------------------------

def _max_dim(gpu):
    return int(gpu.load().smcmc_max_perchain_dim())


def _per_chain(gpu, n, kernel, case_list):
    # 70 chains: the first, one of the ragged tail behind the 64th, the last.  Above 63 dimensions (one chain per
    # workgroup, no tail) five chains: every chain that fails runs the host ladder, whose Jacobi costs O(100 n^3).
    nchains = 70 if n <= 63 else 5
    which = (0, 65 if nchains == 70 else 2, nchains - 1)
    for case in case_list:
        A = case.A if isinstance(case, T.Case) else case
        if kernel == "workgroup":
            e = gpu.Engine(n, nchains, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)
            assert e.get_param("PERCHAIN_WORKGROUP") == 1
        else:
            e = gpu.Engine(n, nchains, mode=gpu.MODE_PER_CHAIN)
            e.set_param("PERCHAIN_WAVE", 1 if kernel == "wave" else 0)
            assert e.get_param("PERCHAIN_WAVE") == (1 if kernel == "wave" else 0)
        assert e.Start(np.zeros(n))
        e.SetCovariance(A)
        e.SetCovarianceFrozen(True)
        e.SetCovarianceWindow(10 ** 6)
        e.SetCovarianceTrials(1e6)
        e.SetNextUpdate(2)                               # UpdateState counts a move at the start of the following step:
        updates = e.lane("update_count").copy()          # none in step 1, one each in steps 2 and 3 (metropolis = 2:
        e.Step(3, 2)                                     # every proposal is taken), so the third step updates
        assert np.all(e.lane("update_count") == updates + 1), case
        paths, full = e.lane("last_update_path"), e.lane("decomp_full")
        assert np.all(paths == paths[0]) and np.all(full == full[0]), case
        for c in which:
            _, cov, dec = e.chain_proposal(c)
            tag = f"{kernel} {case if isinstance(case, T.Case) else 'non-finite'} chain {c}"
            if isinstance(case, T.Case):
                T.check_ladder(case, int(paths[c]), bool(full[c]), cov, dec, tag)
            else:
                assert paths[c] >= 1 and np.all(np.isfinite(dec)), tag
        e.close()


@pytest.mark.parametrize("n", [2, 31, 63])
@pytest.mark.parametrize("kernel", ["lane", "wave"])
def test_per_chain_lane_and_wave_kernels(gpu, kernel, n):
    """One chain per lane (PERCHAIN_WAVE = 0) and per wavefront: the frozen covariance is the injected matrix, bit for
    bit where the plain decomposition takes it; the failing member of the decision pair (g) and the matrices that are
    not positive definite stop the chain for the host ladder (last_update_path >= 1), whose result is judged too."""
    _per_chain(gpu, n, kernel, cases(n) + [nan_case(n)])


@pytest.mark.parametrize("n", [2, 63, 64, 65, 100, "max"])
def test_per_chain_workgroup_kernel(gpu, n):
    """One chain per workgroup, up to smcmc_max_perchain_dim()."""
    n = _max_dim(gpu) if n == "max" else n
    _per_chain(gpu, n, "workgroup", cases(n) + [nan_case(n)])


# ---- the Cholesky chain ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 64, 129])
def test_cholesky_chain_factor(gpu, n):
    """smcmc_cholesky_chain's decomposition (2 slots): the residual bound, and SMCMC_ERR_RUNTIME where the decision says
    the matrix has no factor or an entry is not finite."""
    mean = np.zeros(n)
    for case in cases(n):
        try:
            _, U = gpu.cholesky_chain(mean, case.A, 2, NCHAINS)
            ok = True
        except gpu.SmcmcError:
            ok = False
        T.check_cholesky_decision(case, ok)
        if ok:
            T.cholesky_residual(case.A, U, f"cholesky_chain {case}")
    for A in T.non_finite(n):
        with pytest.raises(gpu.SmcmcError):
            gpu.cholesky_chain(mean, A, 2, NCHAINS)


# ---- HMC: Householder + QL on the device ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 5, 62, 63, 64, 65, 130])
def test_hmc_error_matrix_eigenvalues(gpu, n):
    """pc_eigenvalues and the repair loop through smcmc_selftest_hmc_error_matrix(device = 0): eigenvalues to K n u
    ||A||_2 with K = 53.76 = 32 x 1.68 (numpy.linalg.eigvalsh's worst on the set), the positive / negative decision,
    maxScale, minScale with their clamps and the orbit length.  62, 63, 64: one under, at and one over kPcLdsDim, where
    the matrix image moves from LDS to scratch."""
    for case in T.hmc_cases(n):
        est = float(np.abs(np.diag(case.A)).sum())
        rep, eig, t = gpu.selftest_hmc_error_matrix(case.A, est, device=0)
        sp = case.spectrum()
        tag = f"device {case}"
        if t["passes"] == 0:
            T.ql_eigenvalues(eig, sp, T.K_QL, tag)
        else:
            assert np.array_equal(np.sort(eig), np.sort(np.diag(rep))), tag
        T.hmc_decision_and_scales(case.A, est, rep, t["passes"], t["max_scale"], t["min_scale"], t["orbit"], sp, T.K_QL, tag)
