"""The per-chain HMC mode's entry points without a device: bound, exported, and refusing a null engine."""
import ctypes

NEW = ("smcmc_hmc_set_mode", "smcmc_hmc_get_mode", "smcmc_hmc_read_chain_tuning", "smcmc_selftest_hmc_error_matrix")


def test_new_symbols_are_bound_and_exported(smcmc):
    lib = ctypes.CDLL(smcmc.LIB_PATH)
    for name in NEW:
        assert name in smcmc.SIGNATURES
        assert hasattr(lib, name)


def test_null_engine_is_invalid(smcmc):
    lib = smcmc.load()
    assert lib.smcmc_hmc_set_mode(None, smcmc.MODE_PER_CHAIN) == 1      # SMCMC_ERR_INVALID
    assert lib.smcmc_hmc_set_mode(None, smcmc.MODE_POOLED) == 1
    assert lib.smcmc_hmc_get_mode(None) == -1
    assert lib.smcmc_hmc_read_chain_tuning(None, 0, None, None, None) == 1


def test_error_matrix_host_routine(smcmc):
    """device < 0 is the host routine: the repair loop turns an indefinite matrix into a positive diagonal one"""
    import numpy as np
    cov = np.array([[1.0, 2.0], [2.0, 1.0]])
    rep, eig, t = smcmc.selftest_hmc_error_matrix(cov, 2.0, device=-1)
    assert t["passes"] == 1
    assert np.array_equal(rep, np.eye(2)) and np.array_equal(eig, [1.0, 1.0])
    # the scales run over every pass (:764-791): eigenvalues 3 and -1 first, then 1 and 1
    assert t["trace"] == 2.0 and t["max_scale"] == np.sqrt(3.0) and abs(t["min_scale"] - 1.0) < 1e-15
