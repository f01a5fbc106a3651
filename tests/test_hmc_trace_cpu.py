"""The HMC trace surface without a GPU: smcmc_hmc_step_save, smcmc_hmc_step_recorded, smcmc_hmc_record_stride,
smcmc_hmc_snapshot and smcmc_hmc_rollback answer a NULL handle, the Python field list is the header's enum, and the
programs that use the new surface compile."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "root-simple-mcmc_amd", "lib")
INVALID = 1


def test_null_handle_is_invalid(smcmc):
    lib = smcmc.load()
    assert lib.smcmc_hmc_step_save(None, 1, 1, None, None) == INVALID
    assert lib.smcmc_hmc_step_recorded(None, 1, 0, None) == INVALID
    assert lib.smcmc_hmc_snapshot(None) == INVALID
    assert lib.smcmc_hmc_rollback(None) == INVALID


def test_record_stride_of_null_is_zero(smcmc):
    assert smcmc.load().smcmc_hmc_record_stride(None) == 0


def test_record_fields_are_the_headers_enum(smcmc):
    text = open(os.path.join(ROOT, "include", "smcmc.h")).read()
    m = re.search(r"typedef enum \{([^}]*)\} smcmc_hmc_record_field;", text)
    assert m, "smcmc_hmc_record_field is not in include/smcmc.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = re.findall(r"SMCMC_HMC_REC_(\w+)", body)
    # ..., TUNING0, COUNT_ = SMCMC_HMC_REC_TUNING0 + 10
    assert names[-3:] == ["TUNING0", "COUNT_", "TUNING0"] and re.search(r"COUNT_\s*=\s*SMCMC_HMC_REC_TUNING0\s*\+\s*10", body)
    scalars = [n.lower() for n in names[:-3]]
    from root_simple_mcmc_amd import _capi
    assert smcmc.HMC_RECORD_FIELDS == scalars + _capi.HMC_TUNING
    assert len(_capi.HMC_TUNING) == 10 and scalars[0] == "potential"
    assert re.search(r"#define SMCMC_HMC_RUN_AHEAD 1\b", open(os.path.join(ROOT, "include", "TSimpleHMC_amd.H")).read())


def _compile(source, tmp_path):
    exe = str(tmp_path / (os.path.basename(source) + ".exe"))
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, source),
           f"-L{LIBDIR}", "-lsmcmc_amd", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_step_loop_example_compiles(smcmc, tmp_path):
    _compile(os.path.join("examples", "HmcStepLoop_amd.C"), tmp_path)


def test_run_ahead_driver_compiles(smcmc, tmp_path):
    _compile(os.path.join("tests", "cpp", "hmc_run_ahead.C"), tmp_path)
