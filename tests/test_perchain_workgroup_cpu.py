"""SMCMC_P_PERCHAIN_WORKGROUP (SMCMC_MODE_PER_CHAIN above dimension 63, one chain per workgroup): the C ABI, the
binding and the Python keyword, without a GPU."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "smcmc.h")).read()


def test_the_parameter_is_appended_after_the_others(smcmc):
    from importlib import import_module
    capi = import_module(smcmc.__name__ + "._capi")
    assert capi.P["PERCHAIN_WORKGROUP"] == 26
    assert capi.P["PERCHAIN_WAVE"] == 25                          # nothing before it moved
    assert re.search(r"SMCMC_P_PERCHAIN_WORKGROUP\s*=\s*26\s*,", _header())
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"SMCMC_P_PERCHAIN_WAVE\s*=\s*25\s*,\s*SMCMC_P_PERCHAIN_WORKGROUP\s*=\s*26\s*,\s*SMCMC_P_COUNT_", text)


def test_largest_perchain_dimension(smcmc):
    assert re.search(r"int\s+smcmc_max_perchain_dim\s*\(\s*void\s*\)\s*;", _header())
    assert "smcmc_max_perchain_dim" in smcmc.SIGNATURES
    for path in (smcmc.LIB_PATH, smcmc.FROZEN_DEFINITION_LIB_PATH):
        lib = ctypes.CDLL(path)
        lib.smcmc_max_perchain_dim.restype = ctypes.c_int
        assert lib.smcmc_max_perchain_dim() >= 150
        lib.smcmc_max_register_dim.restype = ctypes.c_int
        assert lib.smcmc_max_register_dim() == 63               # the register-resident kernels are what they were


def test_engine_takes_the_keyword(smcmc):
    sig = inspect.signature(smcmc.Engine.__init__)
    assert "perchain_workgroup" in sig.parameters
    assert sig.parameters["perchain_workgroup"].default is False
