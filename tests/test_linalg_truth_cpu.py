"""The host's dense factorisations against an independent truth (tests/linalg_truth.py): SharedProposal's Cholesky
decomposition and ladder, its cyclic Jacobi, HmcShared's Householder + QL eigenvalues, scales and Gauss-Jordan inverse,
through the stand-alone tests/cpp/linalg_host.C, and the oracle's restatements of the first two.  The verdicts are
rounding-error bounds from the literature, not a comparison of one restatement with another; the last tests show that
they reject small mutations of plain-Python versions of each routine."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER_SIZES = tuple(n for n in T.SIZES if n <= 65)

K_EIGEN, K_QL, KS_INVERSE = T.K_EIGEN, T.K_QL, T.KS_INVERSE
check_cholesky_decision, check_ladder = T.check_cholesky_decision, T.check_ladder


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    work = tmp_path_factory.mktemp("linalg_host")
    exe = T.build_harness(ROOT, work)
    return lambda records: T.run_harness(exe, work, records)


@pytest.fixture(scope="module")
def cholesky_runs(harness):
    cases = [c for n in T.SIZES for c in T.cholesky_cases(n)]
    out = harness([(0, c.A, 0.0, 0.0) for c in cases])
    return {c.name: (c, o) for c, o in zip(cases, out)}


def ladder_cases(n):
    extra = T.decision_pair(n, 1e-10, graded_by=0) if n > T.SOLVE_LIMIT else []     # a pair with a known spectrum
    return T.cholesky_cases(n) + extra + [T.over_correlated(n)]


@pytest.fixture(scope="module")
def ladder_runs(harness):
    cases = [c for n in LADDER_SIZES for c in ladder_cases(n)]
    out = harness([(1, c.A, 0.0, 0.0) for c in cases])
    return list(zip(cases, out))


@pytest.fixture(scope="module")
def hmc_runs(harness, smcmc):
    cases = [c for n in T.SIZES for c in T.host_hmc_cases(n)]
    est = [float(np.abs(np.diag(c.A)).sum()) for c in cases]
    out = harness([(2, c.A, e, 1e6) for c, e in zip(cases, est)])
    runs = []
    for c, e, o in zip(cases, est, out):
        rep, eig, tuning = smcmc.selftest_hmc_error_matrix(c.A, e, device=-1)        # the eigenvalues and the pass count
        runs.append((c, e, o, rep, eig, tuning))
    return runs


def test_constructed_spectra_are_exact():
    """The constructed matrices are V diag(values) V^T with orthonormal V, to the last bit of np.longdouble; and at a
    size mpmath still solves quickly the constructed spectrum is what mpmath finds."""
    for n in (63, 64, 65, 96, 129):
        for case in (T.geometric(n, 10), T.single_small(n), T.thirds(n), T.halves_one_negative(n), T.two_negatives(n)):
            sp = case.spectrum(vectors=True)
            assert sp.exact
            lam = np.array([T.mp_to_ld(v) for v in sp.values])
            V = sp.vectors
            assert T._fro((V.T * lam) @ V - T._ld(case.A)) <= n * 2.0 ** -62 * T._fro(case.A), case
            assert T._fro(V @ V.T - np.eye(n)) <= n * 2.0 ** -62, case
    A, sp = T.constructed([T.Fraction(1, 2 ** (i % 11)) for i in range(33)] + [T.Fraction(-1, 128)], 5)
    solved = T.solve(A)
    assert max(abs(a - b) for a, b in zip(solved.values, sp.values)) < 1e-40


@pytest.mark.parametrize("n", T.SIZES)
def test_host_cholesky(cholesky_runs, n):
    """SharedProposal::choleskyOnly on every family.  Worst observed fraction of the componentwise bound: 0.44 (d-graded,
    n = 2: 0.443); 0.16 at n >= 31."""
    for case in T.cholesky_cases(n):
        case, got = cholesky_runs[case.name]
        check_cholesky_decision(case, got["ok"])
        if got["ok"]:
            T.cholesky_residual(case.A, got["decomp"], str(case))


def test_host_cholesky_refuses_non_finite_entries(harness):
    mats = [A for n in (2, 5, 33, 65) for A in T.non_finite(n)]
    for A, got in zip(mats, harness([(0, A, 0.0, 0.0) for A in mats])):
        assert not got["ok"]
    for A, got in zip(mats, harness([(1, A, 0.0, 0.0) for A in mats])):
        assert got["path"] >= 1 and np.all(np.isfinite(got["decomp"]))


@pytest.mark.parametrize("n", LADDER_SIZES)
def test_host_ladder(ladder_runs, n):
    """SharedProposal::finishUpdateOnHost(1.0): whichever rung it ends on, the decomposition is judged against the
    covariance it left.  The eigen rung (path 2, the cyclic Jacobi) with K = 450 (100 x LAPACK's worst 4.50, see
    K_EIGEN): the Jacobi's own worst is 87 n u ||C||_F, 0.19 of the bound (g-decision-minus, n = 64, n - 1 equal
    eigenvalues; 27.7 on c-halves-negative, n = 33: inside a cluster its stopping rule `off > 0` never fires and all
    100 sweeps run)."""
    seen = set()
    for case, got in ladder_runs:
        if case.n != n:
            continue
        assert got["status"] == 0, case
        check_ladder(case, got["path"], got["full"], got["cov"], got["decomp"], str(case))
        seen.add(got["path"])
    assert {0, 1} <= seen and (n < 3 or 2 in seen)


@pytest.mark.parametrize("n", LADDER_SIZES)
def test_oracle_cholesky_and_eigen(oracle, n):
    """The oracle's restatements under the same verdicts: oracle.cholesky on every family, oracle.eigen through the
    ladder's formula on the matrices that are not positive definite."""
    for case in ladder_cases(n):
        ok, Udec = oracle.cholesky(case.A)
        check_cholesky_decision(case, ok)
        if ok:
            T.cholesky_residual(case.A, Udec, f"oracle {case}")
        elif case.solvable:
            val, vec = oracle.eigen(case.A)
            assert np.all(val[1:] <= val[:-1]), case
            T.eigen_rung(case.A, T.rung_from_eigensystem(val, vec), case, K_EIGEN, f"oracle {case}")


@pytest.mark.parametrize("n", T.SIZES)
def test_host_ql_eigenvalues_and_scales(hmc_runs, n):
    """HmcShared's eigenvalues (through smcmc_selftest_hmc_error_matrix, device = -1), decision, scales and orbit length
    (through the harness, whose numbers must be the selftest's).  K = 53.76 = 32 x 1.68, numpy.linalg.eigvalsh's worst
    on the set (tests/linalg_truth.py); the routine's own worst is 1.64 n u ||A||_2, 0.03 of the bound.  Every family
    with an eigenvalue truth, (e) with its n - 1 equal eigenvalues included; d-graded has none above n = 65."""
    for case, est, got, rep, eig, tuning in hmc_runs:
        if case.n != n:
            continue
        tag = str(case)
        assert np.array_equal(rep, got["cov"]) and tuning["max_scale"] == got["max_scale"], tag
        assert tuning["min_scale"] == got["min_scale"] and tuning["orbit"] == got["orbit"], tag
        assert tuning["trace"] == got["est_trace"], tag
        assert got["orbit"] == 2.0 * 3.14 * got["max_scale"], tag
        if not case.solvable:                            # d-graded above n = 65: no eigenvalue truth
            continue
        sp = case.spectrum()
        if tuning["passes"] == 0:
            T.ql_eigenvalues(eig, sp, K_QL, tag)
        else:                                            # the eigenvalues of the last pass: the repaired diagonal's own
            assert np.array_equal(np.sort(eig), np.sort(np.diag(rep))), tag
        T.hmc_decision_and_scales(case.A, est, rep, tuning["passes"], got["max_scale"], got["min_scale"], got["orbit"],
                                  sp, K_QL, tag)


@pytest.mark.parametrize("n", T.SIZES)
def test_host_inverse(hmc_runs, n):
    """HmcShared::invert on the covariance finishUpdate() left (the matrix itself, or its repaired diagonal).
    Every family, (e) and the graded one at every size included.  In units of n u ||A||_F ||X||_F: each residual under
    K = 32 x 181 125, the smaller one under 32 x 0.153, the asymmetry under 32 x 0.00765, each 32 x numpy.linalg.inv's
    worst on this module's set, n = 2 ... 129 (tests/linalg_truth.py).  The routine's worst on the same set: ||A X - I||
    15 966 (a-geometric-1e10, n = 65), ||X A - I|| 0.25, the smaller residual 0.12, the asymmetry 0.0013."""
    for case, est, got, rep, eig, tuning in hmc_runs:
        if case.n == n:
            T.inverse(got["cov"], got["error"], *KS_INVERSE, str(case))


# ---- the criteria reject mutations ----------------------------------------------------------------------------------

def _rejected(verdict, *args):
    with pytest.raises(T.Verdict):
        verdict(*args)


@pytest.mark.parametrize("n", [5, 33])
def test_the_cholesky_criterion_rejects_mutations(n):
    for case in (T.well_conditioned(n), T.graded(n)):
        T.cholesky_residual(case.A, T.cholesky_plain(case.A), str(case))
        for mutation in ("entry", "skip", "early-pivot"):
            _rejected(T.cholesky_residual, case.A, T.cholesky_plain(case.A, mutation), f"{case} {mutation}")
    A = T.well_conditioned(n).A
    _rejected(T.cholesky_residual, A, T.cholesky_plain(A).T.copy(), "lower triangular")
    _rejected(T.cholesky_residual, A, -T.cholesky_plain(A), "negative diagonal")


@pytest.mark.parametrize("n", [5, 31])
def test_the_eigen_criterion_rejects_a_flipped_rotation(n):
    for case in (T.halves_one_negative(n), T.two_negatives(n)):
        val, vec = T.jacobi_plain(case.A)
        T.eigen_rung(case.A, T.rung_from_eigensystem(val, vec), case, K_EIGEN, str(case))
        val, vec = T.jacobi_plain(case.A, "sign")
        _rejected(T.eigen_rung, case.A, T.rung_from_eigensystem(val, vec), case, K_EIGEN, f"{case} sign of s")


@pytest.mark.parametrize("n", [5, 33, 129])
def test_the_eigenvalue_criterion_rejects_a_moved_eigenvalue(n):
    for case in (T.geometric(n, 3), T.two_negatives(n)):
        sp = case.spectrum()
        eig = np.linalg.eigvalsh(case.A)
        T.ql_eigenvalues(eig, sp, K_QL, str(case))
        for k in (0, n // 2, n - 1):
            moved = eig.copy()
            moved[k] += 1e-11 * sp.norm2
            _rejected(T.ql_eigenvalues, moved, sp, K_QL, f"{case} eigenvalue {k}")


def test_the_decision_criterion_rejects_a_wrong_decision():
    plus, minus = T.decision_pair(33, 1e-6, graded_by=0)
    est = 33.0
    for case, passes in ((plus, 1), (minus, 0)):
        rep = T.repaired(case.A, est) if passes else case.A
        _rejected(T.hmc_decision_and_scales, case.A, est, rep, passes, 1.0, 0.01, 6.28, case.spectrum(), K_QL, str(case))


@pytest.mark.parametrize("n", [5, 33])
def test_the_inverse_criterion_rejects_a_scaled_row(n):
    case = T.geometric(n, 3) if n == 5 else T.well_conditioned(n)
    T.inverse(case.A, T.inverse_plain(case.A), *KS_INVERSE, str(case))
    _rejected(T.inverse, case.A, T.inverse_plain(case.A, "row"), *KS_INVERSE, f"{case} row")
    X = T.inverse_plain(case.A)
    X[0, n - 1] *= 1 + 1e-9                               # no longer symmetric
    _rejected(T.inverse, case.A, X, *KS_INVERSE, f"{case} asymmetric")
