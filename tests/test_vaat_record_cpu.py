"""The record of smcmc_vaat_step_recorded without a GPU: the Python field names against the enum of include/smcmc.h, and
the host replay of TProposeVAATStep_amd.H (sMCMC::detail::VaatReplay, what Step() serves its caller from while it runs
ahead) fed with rows built from the CPU restatement of the reference: point, widths, acceptances, trial counts and the
two means of GetSigma / GetAcceptance bit for bit at every step."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enum_names():
    text = open(os.path.join(ROOT, "include", "smcmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef enum \{([^}]*)\} smcmc_vaat_record_field;", text).group(1)
    return [n.strip().split("=")[0].strip() for n in body.split(",") if n.strip()]


def test_field_names_are_the_enum(smcmc):
    names = _enum_names()
    assert names[-1] == "SMCMC_VAAT_REC_COUNT_"
    assert [n[len("SMCMC_VAAT_REC_"):].lower() for n in names[:-1]] == smcmc.VAAT_RECORD_FIELDS
    assert len(smcmc.VAAT_RECORD_FIELDS) == 17
    text = open(os.path.join(ROOT, "include", "smcmc.h")).read()
    assert "SMCMC_VAAT_REC_LOGL = 0" in text                         # the enum counts from zero, in this order


def test_host_replay_is_the_reference_chain(smcmc, oracle, tmp_path):
    exe = str(tmp_path / "vaat_replay_host.exe")
    # no library on the link line: the replay is host code of the header alone
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(ROOT, "tests", "cpp", "vaat_replay_host.C"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    dim, nsteps = 9, 60
    col = {name: k for k, name in enumerate(smcmc.VAAT_RECORD_FIELDS)}
    o = oracle.Vaat(1, dim, kind=0, seed=5)
    assert o.start(np.linspace(-0.8, 0.8, dim))
    o.set_acceptance_window(20.0)                                    # widths move within a few visits per dimension
    o.update_proposal()

    def per_chain():
        return (o.x[:, 0].copy(), o.per_dim("sigma")[:, 0].copy(), o.per_dim("acceptance")[:, 0].copy(),
                o.per_dim("acceptance_trials")[:, 0].astype(float))

    nums = [float(dim), float(nsteps)] + [v for a in per_chain() for v in a]
    want = []
    for k in range(nsteps):
        before = int(o.lane("last_index")[0])
        o.step(1)
        x, sigma, acc, trials = per_chain()
        row = np.zeros(len(col))
        for name in ("logl", "logl_proposed", "step_rms", "proposed_value", "last_accept", "trials", "successes", "naccept",
                     "step_rms_trials"):
            row[col[name]] = o.lane(name)[0]
        idx = int(o.lane("last_index")[0])
        row[col["index"]] = idx
        row[col["accepted_value"]] = x[idx]
        row[col["adapt_index"]] = before if before >= 0 else -1
        if before >= 0:
            row[col["adapt_sigma"]], row[col["adapt_acceptance"]], row[col["adapt_trials"]] = sigma[before], acc[before], trials[before]
        row[col["total_steps"]] = k + 1
        row[col["queue_length"]] = o.lane("queue_len")[0]
        nums += list(row)
        # GetSigma / GetAcceptance (TProposeVAATStep.H:157-175): the sum in index order, then the division
        mean_sigma, mean_acc = 0.0, 0.0
        for d in range(dim):
            mean_sigma += sigma[d]
            mean_acc += acc[d]
        want.append(np.concatenate([x, sigma, acc, trials, [mean_sigma / dim, mean_acc / dim, o.lane("trials")[0],
                                                           o.lane("successes")[0], o.lane("queue_len")[0]]]))
    r = subprocess.run([exe], input=" ".join(float(v).hex() for v in nums), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == nsteps
    for k, line in enumerate(lines):
        got = np.array([float.fromhex(t) for t in line.split()])
        assert np.array_equal(got, want[k]), (k, np.flatnonzero(got != want[k]))
    assert not np.all(want[-1][dim:2 * dim] == 2.34)                 # the widths did move
    assert len({tuple(w[:dim]) for w in want}) > 5                   # ... and so did the point
