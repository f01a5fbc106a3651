"""SMCMC_P_PERCHAIN_STREAM (SMCMC_MODE_PER_CHAIN from dimension 64 to 512, one chain per workgroup with its matrices
streamed from device memory): the C ABI, the binding, the Python keyword and the kernel's index helpers, without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "root-simple-mcmc_amd", "csrc")
DIMS = (64, 157, 256, 257, 511, 512)


def _header():
    return open(os.path.join(ROOT, "include", "smcmc.h")).read()


def test_the_parameter_is_appended_after_the_others(smcmc):
    from importlib import import_module
    capi = import_module(smcmc.__name__ + "._capi")
    assert capi.P["PERCHAIN_STREAM"] == 27
    assert capi.P["PERCHAIN_WORKGROUP"] == 26                     # nothing before it moved
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    # SMCMC_P_COUNT_ keeps its place behind 26 and counts the parameter that follows it
    assert re.search(r"SMCMC_P_PERCHAIN_WORKGROUP\s*=\s*26\s*,\s*SMCMC_P_COUNT_\s*=\s*28\s*,\s*SMCMC_P_PERCHAIN_STREAM\s*=\s*27\s*}", text)
    assert len(capi.PARAMS) == 28


def test_largest_streamed_dimension(smcmc):
    assert re.search(r"int\s+smcmc_max_perchain_stream_dim\s*\(\s*void\s*\)\s*;", _header())
    assert "smcmc_max_perchain_stream_dim" in smcmc.SIGNATURES
    for path in (smcmc.LIB_PATH, smcmc.FROZEN_DEFINITION_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in ("smcmc_max_perchain_stream_dim", "smcmc_max_perchain_dim", "smcmc_max_dim"):
            getattr(lib, name).restype = ctypes.c_int
        assert lib.smcmc_max_perchain_stream_dim() == lib.smcmc_max_dim() == 512
        assert lib.smcmc_max_perchain_dim() == 156               # without the parameter the mode is what it was


def test_engine_takes_the_keyword(smcmc):
    sig = inspect.signature(smcmc.Engine.__init__)
    assert "perchain_stream" in sig.parameters
    assert sig.parameters["perchain_stream"].default is False


def test_index_helpers_on_the_host(tmp_path):
    """tests/cpp/perchain_stream_index.C: the kernel's own index helpers, compiled without HIP and with the address and
    undefined-behaviour sanitizers, over every packed slot of the dimensions where the kernel takes another path."""
    exe = str(tmp_path / "perchain_stream_index.exe")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "perchain_stream_index.C"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + [str(d) for d in DIMS], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"dims {len(DIMS)} failures 0 max_dim 512" in r.stdout
